// oa_cluster.hpp -- DBSCAN on a point-cloud target: the connected components of the radius graph over the core vertices, border
// vertices attached, labels, sizes and the keep mask (oa_target_clusters).
//
// The contract, with r2 = (float)eps * (float)eps and d2_metric the float32 metric of the searches:
//   count_i = #{ j : d2_metric(v_i, v_j) <= r2 } (self and duplicates count; a vertex with a non-finite coordinate counts 0 and is
//   counted by nobody); core_i = count_i >= min_points; two core vertices are linked iff d2_metric <= r2; a cluster is a connected
//   component of the core graph, numbered 0, 1, ... by ascending lowest core index; a non-core vertex with a core vertex within
//   the radius is a border vertex of the lowest-numbered such cluster; everything else is noise, label -1.
// d2_metric is SYMMETRIC bit for bit -- its differences change sign with the arguments' order, their squares do not, and the
// three squares are added in the same order -- so the graph is undirected, and so is the pruning (bvh_prune against the same r2,
// oa_outlier.hpp's exactness argument: a vertex of a skipped box has d2 > r2 strictly).
//
//   k_bvh_radius_count<true>  (oa_outlier.hpp, as it is) with cap = min_points: count saturates at min_points, so core_i = count_i >=
//                    min_points and count_i <= 1 marks a vertex nobody but itself is near.
//   k_bvh_cluster<CL_LINK>    k_bvh_radius_count's launch shape and walk (bvh_radius_walk, oa_outlier.hpp): one wave per leaf, the
//                    leaf's vertices as queries one after the other, every hit one evaluation of d2_metric.  Only CORE queries descend.  At a
//                    visited leaf the lanes whose vertex is a hit, is core and has a LOWER index than the query are joined with
//                    the query.  Lower index alone suffices: the edge {i, j}, j < i, is seen by query i (metric and pruning are
//                    symmetric), so every edge is linked exactly once.  Joining is oa_unionfind.hpp's lock-free union-find on
//                    parent[nt]: relaxed agent-scope loads, compare-and-swap to hook, atomic minimum to compress; no plain store
//                    to parent in this launch, no wave waits for another, every loop bounded by a budget of steps that raises
//                    ClusterStats::err instead of spinning.  The per-XCD L2s need not agree within a launch: correctness rests on
//                    the compare-and-swap alone (oa_unionfind.hpp says why a stale parent is harmless).  Per visited leaf the hit
//                    lanes resolve their roots, the query its running root, the wave takes the minimum, and only lanes whose root
//                    differs from it issue a compare-and-swap.
//   k_cluster_flatten         a separate launch, so plain loads see the finished forest: root_i for every core vertex = the
//                    LOWEST core index of its component, whichever order the waves ran in.
//   k_bvh_cluster<CL_BORDER>  the same walk for the non-core queries with count >= 2: border_root_i = the minimum of root_j
//                    over the core hits, a wave minimum per leaf, no atomics.  Labels ascend with the root, so the lowest root is
//                    the lowest label.
//   k_cluster_label / _largest / _keep   dense labels from the scan of the root flags (scan_counts_ll: ascending root order), sizes
//                    by integer atomicAdd, the largest cluster by a fixed-order argmax (greatest size, then lowest label), the
//                    keep flags; k_outlier_compact compacts.
// Integer atomics and comparisons only: two calls give the same bits.
#pragma once
#include "oa_outlier.hpp"
#include "oa_unionfind.hpp"

namespace oa {

constexpr int CL_LINK = 0, CL_BORDER = 1;                            // k_bvh_cluster's MODE
constexpr int CL_THREADS = 256;                                      // the plain kernels
constexpr int CL_KEEP_CLUSTERED = 0, CL_KEEP_LARGEST = 1, CL_KEEP_MIN_SIZE = 2;      // OA_CLUSTER_KEEP_*

// zeroed before the call, read back once at its end
struct ClusterStats {
    unsigned long long n_core, n_border, n_noise, n_nonfinite;       // n_noise: every vertex of label -1, the non-finite ones included
    long long n_clusters, largest_label, largest_size;
    int err, pad;                                                    // a union-find budget ran out (never seen)
};

#if defined(__HIPCC__)

struct UfDeviceAtomics {
    static __device__ __forceinline__ uint32_t load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ uint32_t cas(uint32_t *p, uint32_t want, uint32_t v) { return atomicCAS(p, want, v); }
    static __device__ __forceinline__ void fetch_min(uint32_t *p, uint32_t v) { atomicMin(p, v); }
};

// Launch: 64 * KNN_WPB threads (or fewer whole waves), any number of workgroups (the leaves are dealt wave by wave, grid stride).
// count: k_bvh_radius_count<true>(cap = min_points).  max_steps: the union-find budget of one lane at one visited leaf.
// CL_LINK:   parent (nt, parent[i] = i before the launch) is joined; root / border_root are not touched.
// CL_BORDER: root (k_cluster_flatten) is read, border_root[qi] written for every query that descends (the others keep what the
//            host's memset left: IDX_NONE); parent is not touched.
template <int MODE>
__global__ __launch_bounds__(KNN_WPB * 64) void k_bvh_cluster(BvhParams bp, const float4 *__restrict__ boxes, const float4 *__restrict__ prims, float r2,
                                                              int min_points, const int32_t *__restrict__ count, uint32_t *parent,
                                                              const uint32_t *__restrict__ root, uint32_t *__restrict__ border_root, int max_steps,
                                                              ClusterStats *__restrict__ st)
{
    __shared__ unsigned long long s_mask[KNN_WPB][BVH_MAX_LEVELS + 1];
    __shared__ int s_node[KNN_WPB][BVH_MAX_LEVELS + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const BvhLds lds{ nullptr, 0, &s_mask[w][0], 1, &s_node[w][0], 1 };      // (no bounds: nothing is ordered by them)
    bool spent = false;

    for (int leaf = blockIdx.x * wpb + w; leaf < bp.cnt[1]; leaf += gridDim.x * wpb) {     // (wave-uniform)
        const float4 mine = prims[(long long)leaf * BVH_W + lane];
        const uint32_t my_idx = __float_as_uint(mine.w);
        for (int q = 0; q < BVH_W; ++q) {
            uint32_t qi; float p[3];
            if (!knn_leaf_query(mine, my_idx, q, qi, p)) break;
            const int qc = count[qi];                                // (wave-uniform; 0 for a non-finite query)
            if (MODE == CL_LINK ? qc < min_points : (qc >= min_points || qc < 2)) continue;
            uint32_t qr = MODE == CL_LINK ? qi : IDX_NONE;            // LINK: the query's running root; BORDER: the lowest root so far
            bvh_radius_walk(bp, boxes, lds, p, r2, lane, [&](long long child) {
                // leaf: 64 vertices, one per lane
                const float4 c4 = prims[child * BVH_W + lane];
                const float d = d2_metric(p[0], p[1], p[2], c4.x, c4.y, c4.z);
                const uint32_t ci = __float_as_uint(c4.w);
                bool hit = d <= r2 && d < INFINITY && ci != IDX_NONE && (MODE == CL_BORDER || ci < qi);
                if (hit) hit = count[ci] >= min_points;              // core
                if (__ballot(hit) == 0ull) return false;
                if (MODE == CL_BORDER) {
                    qr = min(qr, wave_min_u32(hit ? root[ci] : IDX_NONE));
                    return false;
                }
                int budget = max_steps, qbudget = max_steps;
                const uint32_t r = hit ? uf_find_compress<UfDeviceAtomics>(parent, ci, budget) : IDX_NONE;
                qr = (uint32_t)__builtin_amdgcn_readfirstlane((int)uf_find<UfDeviceAtomics>(parent, qr, qbudget));    // (wave-uniform)
                const uint32_t lowest = wave_min_u32(min(r, qr));
                if (hit && r != lowest) uf_link<UfDeviceAtomics>(parent, r, lowest, budget);
                if (lane == 0 && qr != lowest) uf_link<UfDeviceAtomics>(parent, qr, lowest, qbudget);
                qr = lowest;
                spent |= budget <= 0 || qbudget <= 0;
                return false;                                        // (a cluster pass visits every leaf in reach)
            });
            if (MODE == CL_BORDER) { if (lane == 0) border_root[qi] = qr; }
            else if (lane == 0 && qr != qi) atomicMin(&parent[qi], qr);      // (the next query that meets qi walks one step)
        }
    }
    if (MODE == CL_LINK && spent) atomicOr(&st->err, 1);
}

#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
// Launch (this and the kernels below but k_cluster_largest): CL_THREADS threads, ceil(nt / CL_THREADS) workgroups.
__global__ __launch_bounds__(CL_THREADS) void k_cluster_init(int nt, uint32_t *__restrict__ parent)
{
    const long long i = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    if (i < nt) parent[i] = (uint32_t)i;
}

// root_i = the root of core vertex i (IDX_NONE for the others), is_root_i = 1 where a core vertex is its own root.  Plain loads:
// the link pass has ended.  The walk is bounded by nt (parents only fall); a longer one raises st->err.
__global__ __launch_bounds__(CL_THREADS) void k_cluster_flatten(const uint32_t *__restrict__ parent, const int32_t *__restrict__ count, int min_points, int nt,
                                                                uint32_t *__restrict__ root, int *__restrict__ is_root, ClusterStats *__restrict__ st)
{
    const long long i = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    if (i >= nt) return;
    uint32_t r = IDX_NONE;
    if (count[i] >= min_points) {
        r = (uint32_t)i;
        int steps = nt;
        for (uint32_t p = parent[r]; p != r && steps > 0; p = parent[r], --steps) r = p;
        if (steps <= 0) atomicOr(&st->err, 2);
    }
    root[i] = r;
    is_root[i] = r == (uint32_t)i ? 1 : 0;
}

// label_i = dense[root] (dense = the exclusive scan of is_root: clusters in ascending order of their lowest core index) with root =
// root_i for a core vertex, border_root_i for the others; -1 without one.  sizes[label] += 1.  Counts core, border, noise and the
// vertices with a non-finite coordinate (one integer add per workgroup and class); thread 0 stores the number of clusters, dense[nt].  sizes: zeroed, room for nt.
__global__ __launch_bounds__(CL_THREADS) void k_cluster_label(const uint32_t *__restrict__ root, const uint32_t *__restrict__ border_root,
                                                              const long long *__restrict__ dense, const float *__restrict__ xyz, int nt,
                                                              int32_t *__restrict__ label, int32_t *__restrict__ sizes, ClusterStats *__restrict__ st)
{
    const long long i = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    bool core = false, border = false, noise = false, bad = false;
    int32_t l = -1;
    if (i < nt) {
        const uint32_t r = root[i], b = border_root[i];
        core = r != IDX_NONE;
        border = !core && b != IDX_NONE;
        noise = !core && !border;
        l = core ? (int32_t)dense[r] : (border ? (int32_t)dense[b] : -1);
        label[i] = l;
        bad = !(fabsf(xyz[3 * i]) < INFINITY && fabsf(xyz[3 * i + 1]) < INFINITY && fabsf(xyz[3 * i + 2]) < INFINITY);
        if (i == 0) st->n_clusters = dense[nt];
    }
    // sizes: one add per WORKGROUP when all its vertices carry one label (a cloud that is one object would otherwise send every
    // vertex's add to one word), else one per wave and label -- the lanes that share the first waiting lane's label go together.
    // (Every thread of the workgroup reaches the barriers: nothing above returns.)
    __shared__ int32_t s_l0;
    if (threadIdx.x == 0) s_l0 = l;
    __syncthreads();
    const int32_t l0 = s_l0;
    if (__syncthreads_count(l == l0 ? 1 : 0) == (int)blockDim.x && l0 >= 0) {
        if (threadIdx.x == 0) atomicAdd(&sizes[l0], (int32_t)blockDim.x);
    } else {
        for (unsigned long long todo = __ballot(l >= 0); todo;) {
            const int first = __ffsll((long long)todo) - 1;
            const int32_t lf = (int32_t)__builtin_amdgcn_readlane((int)l, first);
            const unsigned long long same = __ballot(l == lf);
            if ((int)(threadIdx.x & 63) == first) atomicAdd(&sizes[lf], (int32_t)__popcll(same));
            todo &= ~same;
        }
    }
    const int nc = __syncthreads_count(core ? 1 : 0), nb = __syncthreads_count(border ? 1 : 0), nn = __syncthreads_count(noise ? 1 : 0),
              nx = __syncthreads_count(bad ? 1 : 0);
    if (threadIdx.x == 0) {
        if (nc) atomicAdd(&st->n_core, (unsigned long long)nc);
        if (nb) atomicAdd(&st->n_border, (unsigned long long)nb);
        if (nn) atomicAdd(&st->n_noise, (unsigned long long)nn);
        if (nx) atomicAdd(&st->n_nonfinite, (unsigned long long)nx);
    }
}

// The largest cluster: greatest size, on equal size the lowest label; (-1, 0) without a cluster.  One workgroup of CL_THREADS:
// thread t takes labels t, t + CL_THREADS, ... in ascending order, a fixed tree in LDS joins the threads.
__global__ __launch_bounds__(CL_THREADS) void k_cluster_largest(const int32_t *__restrict__ sizes, ClusterStats *__restrict__ st)
{
    __shared__ long long s_size[CL_THREADS], s_label[CL_THREADS];
    const long long n = st->n_clusters;
    long long bs = 0, bl = -1;
    for (long long l = threadIdx.x; l < n; l += CL_THREADS) { const long long s = sizes[l]; if (s > bs) { bs = s; bl = l; } }
    s_size[threadIdx.x] = bs; s_label[threadIdx.x] = bl;
    __syncthreads();
    for (int o = CL_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const long long os = s_size[threadIdx.x + o], ol = s_label[threadIdx.x + o];
            if (ol >= 0 && (os > s_size[threadIdx.x] || (os == s_size[threadIdx.x] && (s_label[threadIdx.x] < 0 || ol < s_label[threadIdx.x])))) {
                s_size[threadIdx.x] = os; s_label[threadIdx.x] = ol;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { st->largest_label = s_label[0]; st->largest_size = s_label[0] >= 0 ? s_size[0] : 0; }
}

// keep_i: CLUSTERED label >= 0; LARGEST label = the largest cluster's; MIN_SIZE label >= 0 and sizes[label] >= min_size.  flag: the
// same as ints (what scan_counts_ll takes).
__global__ __launch_bounds__(CL_THREADS) void k_cluster_keep(const int32_t *__restrict__ label, const int32_t *__restrict__ sizes,
                                                             const ClusterStats *__restrict__ st, int mode, long long min_size, int nt,
                                                             int *__restrict__ flag, unsigned char *__restrict__ keep)
{
    const long long i = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    if (i >= nt) return;
    const int32_t l = label[i];
    bool k = l >= 0;
    if (k && mode == CL_KEEP_LARGEST) k = (long long)l == st->largest_label;
    if (k && mode == CL_KEEP_MIN_SIZE) k = (long long)sizes[l] >= min_size;
    flag[i] = k ? 1 : 0;
    keep[i] = k ? 1 : 0;
}
#endif  // !OA_FAMILY_TU

#endif  // __HIPCC__
}  // namespace oa
