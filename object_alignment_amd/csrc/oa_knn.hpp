// oa_knn.hpp -- exact k nearest target vertices of every target vertex, and PCA normals from them.
//
// A point-cloud target has no triangles to take normals from; the plane metric, the normal-angle test and the weighted plane
// metric all need one normal per correspondence.  Everything the estimate needs is resident after the upload: the target in
// Morton order inside the 64-ary box tree (oa_bvh.hpp).  What this header adds is a K-nearest descent (every other search
// here is 1-nearest) and a per-vertex 3 x 3 eigen-solve.
//
//   k_bvh_knn<PCA>   one WAVE per LEAF of the vertex tree; its (up to) 64 queries are the leaf's own vertices, one after the
//                    other -- neighbours in space, so they walk the same boxes and leaves.  Lane j holds the j-th best
//                    (d2, index) of the query so far as one 64-bit key (d2 bits high, original index low: unsigned order =
//                    the library's exact order, lowest index first on ties).  The list starts as the query's own leaf, sorted
//                    by a bitonic network over the wave; the descent is bvh_wave_query's (per level 64 lower bounds in LDS,
//                    children by ascending bound) with the K-TH best as the cut-off.  At a leaf every lane evaluates one
//                    vertex, a ballot finds the keys below the k-th and they are inserted one at a time (every lane
//                    compares, the lanes above the insertion point take their lower neighbour's key).
//                    PCA = false: rows of indices / d2 go out (lane j writes entry j: one coalesced store per query).
//                    PCA = true : the rows are parked in LDS (64 queries x k indices per wave); when the leaf is done LANE q
//                    solves QUERY q -- mean, centred covariance (fp64, both summed in list order), cyclic Jacobi, smallest
//                    eigenpair, sign rule -- so the eigen-solves of a leaf run 64 wide.
//                    The per-query list is knn_wave_list, a __device__ function of its own: k_bvh_knn_score (oa_outlier.hpp) sums
//                    the same list instead of writing it out.
//   k_bbox_finite    bounding box of the finite coordinates (the Morton frame of a tree over a target that has others)
//
// Exactness of the cut-off: a box is skipped only when lb (1 - 1e-5) - 1e-30 > d2_k, d2_k = the k-th best squared distance so
// far (bvh_prune, the 1-nearest test).  lb never exceeds the true bound by more than the margin absorbs and the metric is
// >= D (1 - 5.01u) (oa_bvh.hpp), so every vertex inside has d2 > d2_k STRICTLY: it cannot enter the list, and it cannot tie
// with the k-th either -- a tie on d2 with a lower index is never lost.  d2_k only decreases, so a box skipped once stays out.
#pragma once
#include "oa_bvh.hpp"

namespace oa {

constexpr int KNN_MAX_K = 64;
constexpr int KNN_WPB = 4;                 // most waves per workgroup (k <= 32: 4; larger k: 2 -- the parked rows share 33 KB)
constexpr int KNN_ROWS_INTS = 4 * 64 * 33; // LDS ints of the parked rows: waves x 64 queries x (k | 1) (odd stride: no bank conflicts)
// an empty list entry: d2 = +inf, no index.  Every real entry is smaller (finite d2 >= +0)
constexpr unsigned long long KNN_EMPTY = (0x7F800000ull << 32) | 0xFFFFFFFFull;

inline int knn_waves_per_block(int k) { return k <= 32 ? 4 : 2; }

struct KnnOrient {
    int32_t mode, pad;                     // OA_ORIENT_*
    double p[3];                           // the orient point (TOWARD / AWAY)
};

#if defined(__HIPCC__)

__device__ __forceinline__ float knn_lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ unsigned long long knn_lane_u64(unsigned long long v, int l)   // l wave-uniform
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

// ascending bitonic sort of one key per lane over the 64 lanes (21 compare-exchange steps)
__device__ __forceinline__ unsigned long long knn_wave_sort(unsigned long long key, int lane)
{
#pragma unroll
    for (int k2 = 2; k2 <= 64; k2 <<= 1) {
#pragma unroll
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const unsigned long long other = __shfl_xor(key, j, 64);
            const bool take_min = ((lane & j) == 0) == ((lane & k2) == 0);
            const unsigned long long lo = key < other ? key : other, hi = key < other ? other : key;
            key = take_min ? lo : hi;
        }
    }
    return key;
}

// One rotation of the cyclic Jacobi diagonalisation of a symmetric 3 x 3: zeroes a[P][Q].  Static indices, so that the arrays
// stay in registers (jacobi_rotate, oa_kernels.hpp).  IEEE division and square root: the angle decides the eigenvector here.
template <int P, int Q>
__host__ __device__ inline void sym3_rotate(double a[3][3], double v[3][3])
{
    constexpr int R = 3 - P - Q;
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[P][P] -= t * apq; a[Q][Q] += t * apq;
    a[P][Q] = 0.0; a[Q][P] = 0.0;
    const double arp = a[R][P], arq = a[R][Q];
    a[R][P] = c * arp - s * arq; a[P][R] = a[R][P];
    a[R][Q] = s * arp + c * arq; a[Q][R] = a[R][Q];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 3; ++r) {
        const double vp = v[r][P], vq = v[r][Q];
        v[r][P] = c * vp - s * vq; v[r][Q] = s * vp + c * vq;
    }
}

// PCA of one neighbourhood from its centred sums C = {xx, xy, xz, yy, yz, zz} about vertex (vx, vy, vz): the unit eigenvector
// of the smallest eigenvalue, signed by `orient`, rounded once to float32; curvature l0 / (l0 + l1 + l2).  Degenerate
// (l1 <= 1e-12 l2, l2 zero or not finite): the zero normal, curvature 0.
__host__ __device__ inline void pca_normal(const double C[6], double vx, double vy, double vz, const KnnOrient &orient, float n_out[3],
                                           float &curv_out)
{
    double a[3][3] = { { C[0], C[1], C[2] }, { C[1], C[3], C[4] }, { C[2], C[4], C[5] } };
    double v[3][3] = { { 1.0, 0.0, 0.0 }, { 0.0, 1.0, 0.0 }, { 0.0, 0.0, 1.0 } };
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]), diag = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]);
        if (!(off > 1e-300) || off <= 1e-18 * diag) break;
        sym3_rotate<0, 1>(a, v);
        sym3_rotate<0, 2>(a, v);
        sym3_rotate<1, 2>(a, v);
    }
    const double e0 = a[0][0], e1 = a[1][1], e2 = a[2][2];
    int j0 = 0;                                                      // the smallest eigenvalue, lowest column on equal values
    if (e1 < e0) j0 = 1;
    if (e2 < (j0 == 0 ? e0 : e1)) j0 = 2;
    const double l0 = j0 == 0 ? e0 : (j0 == 1 ? e1 : e2);
    const double ea = j0 == 0 ? e1 : e0, eb = j0 == 2 ? e1 : e2;     // the other two
    const double l1 = ea < eb ? ea : eb, l2 = ea < eb ? eb : ea;
    n_out[0] = 0.f; n_out[1] = 0.f; n_out[2] = 0.f; curv_out = 0.f;
    if (!(l2 > 0.0) || !(l2 < INFINITY) || !(l1 > 1e-12 * l2)) return;
    double n[3] = { col3(v, 0, j0), col3(v, 1, j0), col3(v, 2, j0) };
    const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(len > 0.0)) return;
    // canonical sign: the component of largest magnitude is positive, lowest axis on equal magnitude
    int m = 0;
    if (fabs(n[1]) > fabs(n[0])) m = 1;
    if (fabs(n[2]) > fabs(m == 0 ? n[0] : n[1])) m = 2;
    double sgn = (m == 0 ? n[0] : (m == 1 ? n[1] : n[2])) < 0.0 ? -1.0 : 1.0;
    if (orient.mode != 0) {
        // TOWARD (1): n . (point - v) >= 0;  AWAY (2): n . (v - point) >= 0
        const double dx = orient.p[0] - vx, dy = orient.p[1] - vy, dz = orient.p[2] - vz;
        double dot = sgn * ((n[0] * dx + n[1] * dy) + n[2] * dz);
        if (orient.mode == 2) dot = -dot;
        if (dot < 0.0) sgn = -sgn;
    }
    const double f = sgn / len;
    n_out[0] = (float)(n[0] * f); n_out[1] = (float)(n[1] * f); n_out[2] = (float)(n[2] * f);
    const double l0c = l0 > 0.0 ? l0 : 0.0, tot = (l0c + l1) + l2;
    curv_out = (float)(l0c / tot);
}

// What a one-wave-per-leaf kernel opens query q with (q wave-uniform; the leaf's 64 vertices are `mine`, one per lane, original
// index my_idx): the query's index and coordinates, broadcast from lane q.  false: padding, which closes the last leaf.
__device__ __forceinline__ bool knn_leaf_query(const float4 &mine, uint32_t my_idx, int q, uint32_t &qi, float p[3])
{
    qi = (uint32_t)__builtin_amdgcn_readlane((int)my_idx, q);
    if (qi == IDX_NONE) return false;
    p[0] = knn_lane_f(mine.x, q); p[1] = knn_lane_f(mine.y, q); p[2] = knn_lane_f(mine.z, q);
    return true;
}

// The list of ONE query by ONE wave (all 64 lanes call it together; p, leaf and k are wave-uniform): lane j returns the j-th best
// key of query p, whose own leaf is `leaf` (its 64 vertices: `mine`, one per lane, original index my_idx).  Entries past the
// last finite distance are KNN_EMPTY.  lds: this wave's scratch (bvh_wave_query's).  1 <= k <= 64.
// r2 (wave-uniform): only vertices with d2_metric <= r2 are listed, +inf = no limit.  A vertex beyond r2 gets the
// empty key where it is evaluated, and the cut-off is min(k-th best, r2) from the start -- r2 itself while the list holds fewer
// than k (the empty key's d2 is +inf).  bvh_prune skips a box only when every vertex inside has d2 > limit STRICTLY (above, and
// oa_outlier.hpp for a fixed r2), so d2 == r2 is never lost.  A candidate's two tests, d <= r2 and d < +inf, are ONE compare
// against r2c = min(r2, FLT_MAX) (a finite d is <= FLT_MAX; +inf and NaN are not): with r2 = +inf it is the test d < +inf that
// stood here before, and the limit is the k-th best itself.
__device__ __forceinline__ unsigned long long knn_wave_list(const BvhParams &bp, const float4 *__restrict__ boxes, const float4 *__restrict__ prims,
                                                            const BvhLds &lds, int leaf, const float4 mine, uint32_t my_idx, const float *p, int k,
                                                            float r2, int lane)
{
    const int top = bp.levels;
    const float r2c = fminf(r2, 3.402823466e+38f);
    // the list starts as the query's own leaf: the cut-off is tight at once
    unsigned long long key;
    {
        const float d = d2_metric(p[0], p[1], p[2], mine.x, mine.y, mine.z);
        key = (d <= r2c && my_idx != IDX_NONE) ? (((unsigned long long)__float_as_uint(d) << 32) | my_idx) : KNN_EMPTY;
        key = knn_wave_sort(key, lane);
    }
    unsigned long long kth = knn_lane_u64(key, k - 1);
    float lim = fminf(__uint_as_float((uint32_t)(kth >> 32)), r2);
    const bool finite = fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY;
    int level = top, node = 0;
    bool fresh = true;
    while (finite) {                                         // (a non-finite query has no finite distance: its list stays empty)
        if (fresh) {
            const long long ch = (long long)node * BVH_W + lane;
            float lb = INFINITY;
            bool pass = false;
            if (ch < bp.cnt[level]) {
                const float4 lo = boxes[2 * ((long long)bp.off[level] + ch)], hi = boxes[2 * ((long long)bp.off[level] + ch) + 1];
                lb = bvh_box_bound<false>(p, lo, hi, 0.0);
                pass = lb < INFINITY && !bvh_prune(lb, lim);
                if (level == 1 && ch == leaf) pass = false;  // the own leaf is in the list already
            }
            lds.lb(level)[lane] = lb;
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
        const bool member = (m >> lane) & 1ull;
        const uint32_t lbits = member ? __float_as_uint(lds.lb(level)[lane]) : 0xFFFFFFFFu;   // bounds are >= +0
        const uint32_t mb = wave_min_u32(lbits);
        if (bvh_prune(__uint_as_float(mb), lim)) {            // the nearest candidate is out: so are the others
            if (lane == 0) *lds.mask(level) = 0ull;
            continue;
        }
        const unsigned long long eq = __ballot(member && lbits == mb);
        const int pick = __ffsll((long long)eq) - 1;
        if (lane == 0) *lds.mask(level) = m & ~(1ull << pick);
        const long long child = (long long)*lds.node(level) * BVH_W + pick;
        if (level > 1) {
            --level;
            node = (int)child;
            fresh = true;
            continue;
        }
        // leaf: 64 vertices, one per lane; those below the k-th key enter the list one at a time
        const float4 c4 = prims[child * BVH_W + lane];
        const float d = d2_metric(p[0], p[1], p[2], c4.x, c4.y, c4.z);
        const uint32_t ci = __float_as_uint(c4.w);
        const unsigned long long ck = (d <= r2c && ci != IDX_NONE) ? (((unsigned long long)__float_as_uint(d) << 32) | ci) : KNN_EMPTY;
        unsigned long long cand = __ballot(ck < kth);
        while (cand) {
            const int b = __ffsll((long long)cand) - 1;
            cand &= cand - 1;
            const unsigned long long cnew = knn_lane_u64(ck, b);
            if (!(cnew < kth)) continue;                     // (the k-th key has moved since the ballot)
            const unsigned long long up = __shfl_up(key, 1, 64);
            if (key > cnew) key = (lane > 0 && up > cnew) ? up : cnew;
            kth = knn_lane_u64(key, k - 1);
        }
        lim = fminf(__uint_as_float((uint32_t)(kth >> 32)), r2);
    }
    return key;
}

// Launch: 64 * knn_waves_per_block(k) threads, any number of workgroups (the leaves are dealt wave by wave, grid stride).
// out_idx / out_d2 (nt x k, the caller's vertex order, original indices; unfilled entries -1 / +inf) may be null.
// PCA: xyz = the target in the caller's order (nt x 3), out_n (nt x 3) / out_curv (nt), each may be null.
// 1 <= k <= 64.  Every real vertex is the query of exactly one (wave, q): every output row is written exactly once.
// r2: the neighbourhood's squared radius (knn_wave_list), +inf = the k nearest however far; a shorter row is padded -1 / +inf.
template <bool PCA>
__global__ __launch_bounds__(KNN_WPB * 64) void k_bvh_knn(BvhParams bp, const float4 *__restrict__ boxes, const float4 *__restrict__ prims,
                                                          int k, float r2, int32_t *__restrict__ out_idx, float *__restrict__ out_d2,
                                                          const float *__restrict__ xyz, KnnOrient orient, float *__restrict__ out_n,
                                                          float *__restrict__ out_curv)
{
    __shared__ float s_lb[KNN_WPB][BVH_MAX_LEVELS + 1][BVH_W];
    __shared__ unsigned long long s_mask[KNN_WPB][BVH_MAX_LEVELS + 1];
    __shared__ int s_node[KNN_WPB][BVH_MAX_LEVELS + 1];
    __shared__ int s_rows[PCA ? KNN_ROWS_INTS : 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const BvhLds lds{ &s_lb[w][0][0], BVH_W, &s_mask[w][0], 1, &s_node[w][0], 1 };
    const int rstride = k | 1;
    int *const rows = PCA ? &s_rows[w * 64 * rstride] : nullptr;
    if (PCA && (w + 1) * 64 * rstride > KNN_ROWS_INTS) return;      // (launched with more waves than the parked rows hold)

    for (int leaf = blockIdx.x * wpb + w; leaf < bp.cnt[1]; leaf += gridDim.x * wpb) {     // (wave-uniform)
        const float4 mine = prims[(long long)leaf * BVH_W + lane];
        const uint32_t my_idx = __float_as_uint(mine.w);
        for (int q = 0; q < BVH_W; ++q) {
            uint32_t qi; float p[3];
            if (!knn_leaf_query(mine, my_idx, q, qi, p)) break;
            const unsigned long long key = knn_wave_list(bp, boxes, prims, lds, leaf, mine, my_idx, p, k, r2, lane);
            if (lane < k) {
                const int32_t ni = (int32_t)(uint32_t)key;           // IDX_NONE -> -1
                if (out_idx) out_idx[(long long)qi * k + lane] = ni;
                if (out_d2) out_d2[(long long)qi * k + lane] = __uint_as_float((uint32_t)(key >> 32));
                if (PCA) rows[q * rstride + lane] = ni;
            }
        }
        if (PCA) {
            // lane q solves query q of this leaf
            OA_WAVE_LDS_FENCE();
            if (my_idx != IDX_NONE) {
                const int *__restrict__ row = rows + lane * rstride;
                double sx = 0.0, sy = 0.0, sz = 0.0;
                int m = 0;
                for (; m < k; ++m) {                                 // the mean of the neighbours, in list order
                    const int id = row[m];
                    if (id < 0) break;
                    sx += (double)xyz[3ll * id]; sy += (double)xyz[3ll * id + 1]; sz += (double)xyz[3ll * id + 2];
                }
                float nrm[3] = { 0.f, 0.f, 0.f }, curv = 0.f;
                if (m >= 3) {
                    const double mx = sx / m, my = sy / m, mz = sz / m;
                    double C[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
                    for (int j = 0; j < m; ++j) {                    // centred products, in list order
                        const int id = row[j];
                        const double dx = (double)xyz[3ll * id] - mx, dy = (double)xyz[3ll * id + 1] - my, dz = (double)xyz[3ll * id + 2] - mz;
                        C[0] += dx * dx; C[1] += dx * dy; C[2] += dx * dz; C[3] += dy * dy; C[4] += dy * dz; C[5] += dz * dz;
                    }
                    pca_normal(C, (double)mine.x, (double)mine.y, (double)mine.z, orient, nrm, curv);
                }
                if (out_n) { out_n[3ll * my_idx] = nrm[0]; out_n[3ll * my_idx + 1] = nrm[1]; out_n[3ll * my_idx + 2] = nrm[2]; }
                if (out_curv) out_curv[my_idx] = curv;
            }
            OA_WAVE_LDS_FENCE();                                     // (the next leaf's rows overwrite these)
        }
    }
}

#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
// per workgroup {min xyz, max xyz} over the FINITE coordinates (k_bbox_partial poisons its box with NaN instead); a workgroup
// that saw none writes +inf / -inf.  Launch: 256 threads, any number of workgroups.
__global__ __launch_bounds__(256) void k_bbox_finite(const float *__restrict__ xyz, int n, float *__restrict__ out /* blocks x 6 */)
{
    __shared__ float red[4][6];
    float b[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        for (int a = 0; a < 3; ++a) {
            const float v = xyz[3 * i + a];
            if (fabsf(v) < INFINITY) { b[a] = fminf(b[a], v); b[3 + a] = fmaxf(b[3 + a], v); }
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            b[a] = fminf(b[a], __shfl_xor(b[a], o, 64));
            b[3 + a] = fmaxf(b[3 + a], __shfl_xor(b[3 + a], o, 64));
        }
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 6; ++a) red[threadIdx.x >> 6][a] = b[a];
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        float v = red[0][a];
        for (int k = 1; k < 4; ++k) v = a < 3 ? fminf(v, red[k][a]) : fmaxf(v, red[k][a]);
        out[blockIdx.x * 6 + a] = v;
    }
}
#endif  // !OA_FAMILY_TU

#endif  // __HIPCC__
}  // namespace oa
