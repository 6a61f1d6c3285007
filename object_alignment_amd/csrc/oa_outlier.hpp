// oa_outlier.hpp -- stray points of a point-cloud target: fixed-radius neighbour counts, mean k-nearest distances, and what
// turns them into a keep mask.
//
// Both searches run on the target's 64-ary box tree with k_bvh_knn's launch shape (oa_knn.hpp): one WAVE per LEAF of the vertex
// tree, the leaf's own vertices are its (up to) 64 queries, one after the other; the per-level scratch in LDS is
// bvh_wave_query's (a mask of children still to visit and the node, per level).
//
//   k_bvh_radius_count<CAPPED>  count_i = min(cap, #{ j : d2_metric(v_i, v_j) <= r2 }), r2 a float32 the host squares once.  Self
//                    and duplicates count; a vertex with a non-finite coordinate counts 0 and is counted by nobody.  A child box
//                    is visited iff !bvh_prune(lb, r2) (bvh_radius_walk below, the one fixed-radius descent; oa_cluster.hpp's
//                    passes walk with it too).  At a leaf every lane evaluates one vertex, a ballot and a popcount
//                    add the hits to a wave-uniform count.  The own leaf is one more leaf.  CAPPED: the query stops descending
//                    once `cap` is reached and reports cap -- whichever order the leaves came in, so two runs give the same bits.
//   k_bvh_knn_score  the statistical filter's score without an nt x k buffer: knn_wave_list with k + 1 entries, then
//                    S = sum of sqrt((double)d2_j) over the m filled entries, in list order, fp64; score = S / (m - 1), +inf for
//                    m < 2.  Lane j takes the root of entry j (IEEE, 64 wide); the sum is wave-uniform.  The query itself adds
//                    exactly 0 (or, pushed out of its own row by more than k duplicates of lower index, every entry is 0), so no
//                    "which entry is me" test, and equal distances add the same terms in any order of their indices.
//
// The rest is plain kernels in the host unit: mean and standard deviation of the finite scores (fp64, two passes, fixed order:
// per-workgroup rows by a butterfly and the waves in order, the rows by one workgroup's fixed tree -- k_deviation / k_dev_finish's
// pattern; no floating-point atomics), the keep flags, and the stable compaction behind scan_counts_ll (oa_sort.hpp).
#pragma once
#include "oa_knn.hpp"

namespace oa {

constexpr int OUT_THREADS = 256;           // k_outlier_rows / _finish / _flags / _compact
constexpr int OUT_MAX_ROWS = 1024;         // per-workgroup rows of one pass (a function of n alone: the sums' order is fixed)
constexpr int OUT_STATISTICAL = 0, OUT_RADIUS = 1;     // OA_OUTLIER_*

struct OutlierStats {
    double sum, mean, ssq, std, threshold;
    long long n_finite;                    // finite scores
    long long n_kept;                      // written by k_outlier_compact
    unsigned long long n_nonfinite;        // vertices with a non-finite coordinate (integer atomics)
};

inline int outlier_rows(long long n)
{
    const long long r = (n + OUT_THREADS - 1) / OUT_THREADS;
    return r < 1 ? 1 : (r > OUT_MAX_ROWS ? OUT_MAX_ROWS : (int)r);
}

#if defined(__HIPCC__)

// The fixed-radius descent of ONE finite query p by ONE wave (all 64 lanes call it together; p and r2 are wave-uniform): every
// leaf whose box may hold a vertex with d2_metric <= r2, the query's own among them, goes to at_leaf(child) in the order visited
// (its 64 vertices: prims[child * BVH_W + lane]); at_leaf returns true to end the query.  lds: this wave's scratch, per level a
// mask of children still to visit and the node; the cut-off never moves, so the children are taken in lane order (no bounds
// parked, no minimum over the wave).
// Exactness of the radius test: a box is skipped only when lb (1 - 1e-5) - 1e-30 > r2 (bvh_prune).  lb never exceeds the true
// squared gap D to the box by more than the margin absorbs and the metric is >= D (1 - 5.01u) for every vertex inside
// (oa_bvh.hpp), so every vertex of a skipped box has d2_metric > r2 STRICTLY: it is not a hit, and d2 = r2 is never lost.  There
// is no "whole box inside the radius" shortcut: every hit is one evaluation of d2_metric by at_leaf, the same float32 the
// brute-force restatement compares.
template <class AtLeaf>
__device__ __forceinline__ void bvh_radius_walk(const BvhParams &bp, const float4 *__restrict__ boxes, const BvhLds &lds, const float *p, float r2, int lane,
                                                AtLeaf &&at_leaf)
{
    const int top = bp.levels;
    int level = top, node = 0;
    bool fresh = true;
    for (;;) {
        if (fresh) {
            const long long ch = (long long)node * BVH_W + lane;
            bool pass = false;
            if (ch < bp.cnt[level]) {
                const float4 lo = boxes[2 * ((long long)bp.off[level] + ch)], hi = boxes[2 * ((long long)bp.off[level] + ch) + 1];
                const float lb = bvh_box_bound<false>(p, lo, hi, 0.0);
                pass = lb < INFINITY && !bvh_prune(lb, r2);
            }
            const unsigned long long m = __ballot(pass);
            if (lane == 0) { *lds.mask(level) = m; *lds.node(level) = node; }
            fresh = false;
        }
        const unsigned long long m = *lds.mask(level);
        if (m == 0ull) {
            if (level == top) break;
            ++level;
            continue;
        }
        const int pick = __ffsll((long long)m) - 1;
        if (lane == 0) *lds.mask(level) = m & (m - 1ull);
        const long long child = (long long)*lds.node(level) * BVH_W + pick;
        if (level > 1) {
            --level;
            node = (int)child;
            fresh = true;
            continue;
        }
        if (at_leaf(child)) break;
    }
}

// Launch: 64 * KNN_WPB threads (or fewer whole waves), any number of workgroups (the leaves are dealt wave by wave, grid stride).
// count: nt, the caller's vertex order; every real vertex is the query of exactly one (wave, q): one store per query.
template <bool CAPPED>
__global__ __launch_bounds__(KNN_WPB * 64) void k_bvh_radius_count(BvhParams bp, const float4 *__restrict__ boxes, const float4 *__restrict__ prims,
                                                                   float r2, int cap, int32_t *__restrict__ count)
{
    __shared__ unsigned long long s_mask[KNN_WPB][BVH_MAX_LEVELS + 1];
    __shared__ int s_node[KNN_WPB][BVH_MAX_LEVELS + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const BvhLds lds{ nullptr, 0, &s_mask[w][0], 1, &s_node[w][0], 1 };      // (no bounds: nothing is ordered by them)

    for (int leaf = blockIdx.x * wpb + w; leaf < bp.cnt[1]; leaf += gridDim.x * wpb) {     // (wave-uniform)
        const float4 mine = prims[(long long)leaf * BVH_W + lane];
        const uint32_t my_idx = __float_as_uint(mine.w);
        for (int q = 0; q < BVH_W; ++q) {
            uint32_t qi; float p[3];
            if (!knn_leaf_query(mine, my_idx, q, qi, p)) break;
            const bool finite = fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY;
            int n = 0;                                               // (wave-uniform)
            if (finite)                                              // (a non-finite query has no finite distance: it counts 0)
                bvh_radius_walk(bp, boxes, lds, p, r2, lane, [&](long long child) {
                    // leaf: 64 vertices, one per lane
                    const float4 c4 = prims[child * BVH_W + lane];
                    const float d = d2_metric(p[0], p[1], p[2], c4.x, c4.y, c4.z);
                    n += __popcll(__ballot(d <= r2 && d < INFINITY && __float_as_uint(c4.w) != IDX_NONE));
                    if (CAPPED && n >= cap) { n = cap; return true; }
                    return false;
                });
            if (lane == 0) count[qi] = n;
        }
    }
}

// Launch: as k_bvh_radius_count (no rows are parked: KNN_WPB waves at every k).  k1 = k + 1 list entries, 2 <= k1 <= 64.
// score: nt doubles, the caller's vertex order, one store per query.
// Not a template, so no explicit instantiation places it: oa_fam_knn.hip (OA_FAMILY_KNN_TU) compiles it, every other unit sees
// the declaration and the linker resolves the launch, as for the `extern` instances of oa_families.hpp.
#if defined(OA_FAMILY_KNN_TU)
__global__ __launch_bounds__(KNN_WPB * 64) void k_bvh_knn_score(BvhParams bp, const float4 *__restrict__ boxes, const float4 *__restrict__ prims, int k1,
                                                                double *__restrict__ score)
{
    __shared__ float s_lb[KNN_WPB][BVH_MAX_LEVELS + 1][BVH_W];
    __shared__ unsigned long long s_mask[KNN_WPB][BVH_MAX_LEVELS + 1];
    __shared__ int s_node[KNN_WPB][BVH_MAX_LEVELS + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const BvhLds lds{ &s_lb[w][0][0], BVH_W, &s_mask[w][0], 1, &s_node[w][0], 1 };

    for (int leaf = blockIdx.x * wpb + w; leaf < bp.cnt[1]; leaf += gridDim.x * wpb) {     // (wave-uniform)
        const float4 mine = prims[(long long)leaf * BVH_W + lane];
        const uint32_t my_idx = __float_as_uint(mine.w);
        for (int q = 0; q < BVH_W; ++q) {
            uint32_t qi; float p[3];
            if (!knn_leaf_query(mine, my_idx, q, qi, p)) break;
            const unsigned long long key = knn_wave_list(bp, boxes, prims, lds, leaf, mine, my_idx, p, k1, INFINITY, lane);
            // the filled entries come first (KNN_EMPTY is the largest key)
            const int m = __popcll(__ballot(lane < k1 && key != KNN_EMPTY));
            const double root = sqrt((double)__uint_as_float((uint32_t)(key >> 32)));
            double S = 0.0;
            for (int j = 0; j < m; ++j) S += __longlong_as_double((long long)knn_lane_u64((unsigned long long)__double_as_longlong(root), j));
            if (lane == 0) score[qi] = m >= 2 ? S / (double)(m - 1) : (double)INFINITY;
        }
    }
}
#else
__global__ void k_bvh_knn_score(BvhParams bp, const float4 *__restrict__ boxes, const float4 *__restrict__ prims, int k1, double *__restrict__ score);
#endif

#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
// One row per workgroup.  PASS 0: {sum of the finite scores, their number}; PASS 1: {sum of (score - st->mean)^2 over them}.
// Thread t of workgroup b takes i = b * OUT_THREADS + t, then every gridDim.x * OUT_THREADS further, in ascending order; a
// butterfly joins the wave, thread 0 the waves in order.  Launch: OUT_THREADS threads, outlier_rows(n) workgroups.
template <int PASS>
__global__ __launch_bounds__(OUT_THREADS) void k_outlier_rows(const double *__restrict__ score, long long n, const OutlierStats *__restrict__ st,
                                                              double *__restrict__ row_sum, long long *__restrict__ row_n)
{
    __shared__ double red_s[OUT_THREADS / 64];
    __shared__ long long red_n[OUT_THREADS / 64];
    const double mean = PASS == 1 ? st->mean : 0.0;
    double s = 0.0;
    long long cnt = 0;
    for (long long i = (long long)blockIdx.x * OUT_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * OUT_THREADS) {
        const double v = score[i];
        if (fabs(v) < (double)INFINITY) {
            if (PASS == 0) s += v;
            else { const double e = v - mean; s += e * e; }
            ++cnt;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); cnt += __shfl_xor(cnt, o, 64); }
    if ((threadIdx.x & 63) == 0) { red_s[threadIdx.x >> 6] = s; red_n[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = red_s[0];
        long long b = red_n[0];
        for (int k = 1; k < OUT_THREADS / 64; ++k) { a += red_s[k]; b += red_n[k]; }
        row_sum[blockIdx.x] = a;
        row_n[blockIdx.x] = b;
    }
}

// One workgroup: thread t adds rows t, t + OUT_THREADS, ... in ascending order, a fixed tree in LDS (stride 128, 64, ... 1) joins
// the threads.  PASS 0: st->sum, n_finite, mean.  PASS 1: st->ssq, std (0 for n_finite < 2), threshold = mean + std_ratio std.
template <int PASS>
__global__ __launch_bounds__(OUT_THREADS) void k_outlier_finish(const double *__restrict__ row_sum, const long long *__restrict__ row_n, int n_rows,
                                                                double std_ratio, OutlierStats *__restrict__ st)
{
    __shared__ double red_s[OUT_THREADS];
    __shared__ long long red_n[OUT_THREADS];
    double s = 0.0;
    long long cnt = 0;
    for (int r = threadIdx.x; r < n_rows; r += OUT_THREADS) { s += row_sum[r]; cnt += row_n[r]; }
    red_s[threadIdx.x] = s; red_n[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = OUT_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { red_s[threadIdx.x] += red_s[threadIdx.x + o]; red_n[threadIdx.x] += red_n[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (PASS == 0) {
            st->sum = red_s[0]; st->n_finite = red_n[0];
            st->mean = red_n[0] > 0 ? red_s[0] / (double)red_n[0] : 0.0;
        } else {
            const long long nf = st->n_finite;
            st->ssq = red_s[0];
            st->std = nf >= 2 ? sqrt(red_s[0] / (double)(nf - 1)) : 0.0;
            st->threshold = st->mean + std_ratio * st->std;
        }
    }
}

// keep_i: STATISTICAL score_i <= st->threshold (a score of +inf never); RADIUS count_i - 1 >= min_neighbors.  flag: the same as
// ints (what scan_counts_ll takes).  Counts the vertices with a non-finite coordinate.  Launch: OUT_THREADS threads, ceil(n /
// OUT_THREADS) workgroups.
__global__ __launch_bounds__(OUT_THREADS) void k_outlier_flags(int method, const double *__restrict__ score, const int32_t *__restrict__ count,
                                                               const float *__restrict__ xyz, int n, int min_neighbors, OutlierStats *__restrict__ st,
                                                               int *__restrict__ flag, unsigned char *__restrict__ keep)
{
    const long long i = (long long)blockIdx.x * OUT_THREADS + threadIdx.x;
    bool bad = false;
    if (i < n) {
        bool k;
        if (method == OUT_STATISTICAL) { const double v = score[i]; k = v < (double)INFINITY && v <= st->threshold; }
        else k = count[i] - 1 >= min_neighbors;
        flag[i] = k ? 1 : 0;
        keep[i] = k ? 1 : 0;
        bad = !(fabsf(xyz[3 * i]) < INFINITY && fabsf(xyz[3 * i + 1]) < INFINITY && fabsf(xyz[3 * i + 2]) < INFINITY);
    }
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&st->n_nonfinite, (unsigned long long)__popcll(m));
}

// off = the exclusive scan of flag (off[n] = the number kept): the kept vertices in ascending index order, and (xyz_out != null)
// their coordinates.  Launch: as k_outlier_flags.
__global__ __launch_bounds__(OUT_THREADS) void k_outlier_compact(const int *__restrict__ flag, const long long *__restrict__ off, int n,
                                                                 const float *__restrict__ xyz, int32_t *__restrict__ kept_index,
                                                                 float *__restrict__ xyz_out, OutlierStats *__restrict__ st)
{
    const long long i = (long long)blockIdx.x * OUT_THREADS + threadIdx.x;
    if (i == 0) st->n_kept = off[n];
    if (i >= n || !flag[i]) return;
    const long long o = off[i];
    kept_index[o] = (int32_t)i;
    if (xyz_out) { xyz_out[3 * o] = xyz[3 * i]; xyz_out[3 * o + 1] = xyz[3 * i + 1]; xyz_out[3 * o + 2] = xyz[3 * i + 2]; }
}
#endif  // !OA_FAMILY_TU

#endif  // __HIPCC__
}  // namespace oa
