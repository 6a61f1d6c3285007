// oa_kernels.hpp -- gfx950 (CDNA4, wave64) device code of the ICP hot path.
//
// One ICP iteration inside the loop (oa_run / oa_iterate) is two launches:
//   search + accumulate   k_nn_search_grid<L, ACC> (oa_grid.hpp), k_bvh_search<TRI, ACC> (oa_bvh.hpp) or, for the modes whose
//                         search has no accumulating form (brute force, triangle grid), the search followed by
//                         k_pair_accumulate_canon: world-space threshold test + fp64 sums (functions/general.py:299-306 fused
//                         with the reductions affine_matrix_from_points needs, :160-167,:181,:208-212), one row of NSUMS
//                         doubles per workgroup, fixed order (bitwise reproducible, no float atomics)
//   k_reduce_solve_update rows -> sums -> 3x3 Kabsch/SVD solve, matrix_world update, convergence ring
//                         (operators/icp_align.py:106-149); across devices k_reduce_post -> k_gather_solve_update (mailboxes)
//                         or k_reduce_partials -> ncclAllReduce -> k_solve_update
// This file: the state (DevState), the float32 "mathutils" arithmetic, the brute-force searches
//   k_nn_search / k_nn_search_filtered   nearest target vertex per source point; target tiles staged through LDS and read
//                         back as wave-uniform (broadcast) ds_read_b128; fp32 VALU bound (docs/HISTORY.md 4.1)
// the pair test and the accumulation helpers (pair_eval, block_store_pair), the row reduction and the solve.
//
// Arithmetic conventions are spelled out in DESIGN.md ("float32 semantics") and are shared bit-for-bit with the
// CPU oracle.  This translation unit is compiled with -ffp-contract=off: every fma below is written explicitly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <type_traits>
#include "oa_pairgap.hpp"
#include "oa_quadgap.hpp"
#include "oa_octgap.hpp"
#include "oa_level0.hpp"

namespace oa {

constexpr int NSUMS = 24;
// layout of the per-iteration sums (all relative to `pivot`, a' = a - pivot, b' = b - pivot):
//   [0..2] sum a'   [3..5] sum b'   [6..14] sum b'_i a'_j (row i, col j)   [15] sum |a'|^2   [16] sum |b'|^2
//   [17] K          [18] sum (d - d_pivot)      [19] sum (d - d_pivot)^2        [20] sum w (0 unless weighted)   [21..23] reserved (0)
// Weighted steps (oa_set_robust / oa_set_source_weights, DevState::weighted): every pair carries w = w_vertex * psi(r); sums
// [0..16] are then weighted, [20] is their mass, and [17..19] stay what they are -- the COUNT of pairs and the plain distances.
constexpr int S_A = 0, S_B = 3, S_H = 6, S_AA = 15, S_BB = 16, S_K = 17, S_D = 18, S_DD = 19, S_W = 20;
// the point-to-plane metric (Chen & Medioni; oa_set_metric) sums a wider row.  Per pair, relative to the same pivot: n = the
// correspondence's unit normal in align-local space, r = n . (a' - b'), J = [a' x n, n] (the row of the linearised step
// x = (omega, t)):
//   [0..20] sum J J^T, upper triangle by rows ((0,0) (0,1) .. (0,5) (1,1) .. (5,5))   [21..26] sum J r   [27] K
//   [28] sum (d - d_pivot)   [29] sum (d - d_pivot)^2   [30] sum r^2   [31] sum w (0 unless weighted)
// Weighted steps: [0..26] are sums of w J J^T and w J r; [27..30] stay unweighted.
// The plane-to-plane metric (Generalized-ICP; OA_METRIC_GICP) fills the same row from J = [-[a']x, I3] (3 x 6), e = a' - b' and
// the pair's 3 x 3 weight W: [0..20] sum w J^T W J, [21..26] sum w J^T W e, [30] sum e^T W e; W = n n^T is the plane row exactly.
constexpr int NSUMS_PLANE = 32;
constexpr int P_JJ = 0, P_JR = 21, P_K = 27, P_D = 28, P_DD = 29, P_RR = 30, P_W = 31;

// the robust losses (oa_set_robust; OA_LOSS_* of oa_icp.h) as weights of an iteratively re-weighted step: psi(r), r >= 0 the
// pair's residual in world units, c the loss's scale.  All three are continuous in r.
constexpr int LOSS_NONE = 0, LOSS_HUBER = 1, LOSS_TUKEY = 2, LOSS_CAUCHY = 3;
__host__ __device__ inline double robust_psi(int loss, double r, double c)
{
    if (loss == LOSS_NONE) return 1.0;
    if (loss == LOSS_HUBER) return r <= c ? 1.0 : c / r;
    const double q = r / c, q2 = q * q;
    if (loss == LOSS_TUKEY) { const double u = 1.0 - q2; return r < c ? u * u : 0.0; }
    return 1.0 / (1.0 + q2);                                        // LOSS_CAUCHY
}

constexpr unsigned long long KEY_EMPTY = ~0ull;
constexpr uint32_t IDX_NONE = 0xFFFFFFFFu;

constexpr int NN_THREADS = 256;
constexpr int TILE_GROUPS = 256;          // groups of 4 targets per LDS tile (1024 targets, 12 KiB)
constexpr int ACC_THREADS = 256;
constexpr int ACC_MAX_BLOCKS = 4096;

struct StepRecord {
    double M[16];
    float  new_mat[16];
    double K, mean_d, std_d, trans, angle;
    double search_ticks;      // wall_clock64 ticks from the end of the previous iteration to the start of k_pair_accumulate
    double exchange_ticks;    // ... from "this device's sums are ready" (end of k_reduce_post / k_reduce_partials) to "the world's sums are in
                              // hand" (the gather's wait is over / the solve behind the all-reduce starts); 0 on one GPU
};

struct DevState {
    float  mx1[16], mx2[16], imx1[16], imx2[16];   // align / base matrix_world and inverses (float32, row-major)
    double pivot[3];
    double thresh, target_d;
    double ring_t[5], ring_r[5];
    int32_t iters, use_target, with_scale, early_exit;
    int32_t n, converged, status, halt;
    int32_t max_records, pad0;
    // conservative-filter data (k_nn_search_filtered): target bbox centre and max |q - centre|
    float  tc[3], pad1;
    double qmax;
    int32_t fax[3], pad2;    // filter axes: fax[0], fax[1] kept by the 2-D score, fax[2] (smallest extent) dropped
    double d_pivot;      // subtracted from the pair distances before summing (previous iteration's mean): keeps
                         // the one-pass variance sum d^2 - K mean^2 free of cancellation
    // Search radius (grid / tree searches only): a query whose nearest primitive is farther than
    // cut_a + cut_b (|x| + |y| + |z|) in base-local space is certain to fail `dist < thresh` (general.py:300), so
    // the search may stop there.  cut_a = +inf switches it off (oa_nn_search, brute-force mode).  See search_cutoff().
    double cut_a, cut_b;
    double local_per_world;   // 1 / sigma_min(mx2): upper bound of |local| / |world| distances (0 = unknown)
    int32_t *host_halt;       // pinned host words {halt, n} mirrored for oa_run (stop enqueuing / stay near the GPU), or nullptr
    // GPU-side timing of the search (no hipEvents in the stream: they cost ~3 us each): k_stamp_start / the solve
    // kernel leave the end of the previous iteration in t_prev_end, k_pair_accumulate its own start in t_acc_start
    unsigned long long t_prev_end, t_acc_start;
    unsigned long long t_xchg_start;  // multi-GPU: when this device's sums of the iteration were ready for the exchange (StepRecord::exchange_ticks)
    // shader cycles and constant-rate ticks one workgroup in the middle of the last k_nn_search_sorted launch lived for: the clock
    // the chip held DURING the search (OA_STAT_SEARCH_CLOCK_MHZ; bench.py prices the measured issue rates at this clock)
    unsigned long long search_clk[2];
    // Shards in the zone where the tree search wins while the pose still moves (stale seeds, long reach) and the grid
    // search once it has settled: both are enqueued every iteration and `tree_turn` says whose turn it is.  Set by the
    // host for the first search (no seeds: tree) and by the solve kernel afterwards, from the same quantity the grid
    // kernels double their budget on: last step's translation + rotation x object size against a fraction of a cell.
    double turn_limit, turn_scale;   // OA_TURN_FRAC (0.1) x cell edge and largest |coordinate| of the grid in use
    int32_t tree_turn;
    int32_t mx2_identity;     // base matrix_world is exactly the identity: mx2 @ v == v bit for bit for finite v (pair_eval)
    // multi-device mailbox exchange: sequence number of this loop's iteration 0 minus one.  It grows from loop to loop
    // (the host adds iters + 2 per loop), so a slot left over from an earlier loop can never be mistaken for a post of
    // this one and the mailboxes never have to be cleared (clearing them would need a cross-device ordering of its own)
    unsigned long long seq_base;
    // Jacobi warm start (rotation_from_covariance): the right singular vectors of the last iteration's covariance.
    // H = sum b a^T ~ R (sum a a^T), so H^T H -- what V diagonalises -- hardly changes from one iteration to the next:
    // started from the last V a solve takes one sweep of small rotations instead of three (8 rotations -> 3).
    double jac_v[9];
    int32_t jac_valid;
    int32_t plane_rank;       // plane metric: eigenvalues the last solve kept (OA_STAT_PLANE_RANK); 0 otherwise
    // weighted steps (oa_set_robust / oa_set_source_weights): off (0) unless a loss or vertex weights are set
    int32_t weighted;         // 1: the pairs carry weights -- the solve takes its mass from S_W / P_W instead of the pair count
    int32_t loss;             // LOSS_*
    double robust_c;          // the loss's scale, world units
    double res_scale;         // plane metric: cbrt(|det mx1[:3,:3]|), align-local residual -> world units (set when the loop starts)
    double weight_sum;        // sum w of the last step; K when weighting is off (OA_STAT_WEIGHT_SUM)
    // the loss's scale from the step's own residuals (oa_set_robust_auto): c = max(robust_mult * q, robust_cmin), q the
    // ceil(robust_p * K_q)-th smallest of the K_q float32 residuals that take part; k_select_scan writes robust_c from them
    // before the accumulation reads it.  robust_p = 0: off, robust_c stays what the host wrote
    double robust_mult, robust_p, robust_cmin;
    double robust_q;          // the last step's order statistic (0 when K_q = 0)
    uint32_t robust_kq;       // ... and how many residuals took part
    uint32_t sel_prefix;      // radix select, between its launches: the key's leading bits found so far ...
    uint32_t sel_rank;        // ... and the 0-based rank wanted among the keys that share them
    uint32_t pad3;
    double gicp_eps;          // GICP metric (oa_set_gicp): the covariances' small eigenvalue, C = I - (1 - eps) n n^T; set when the loop starts
    int32_t symmetric;        // symmetric metric (OA_METRIC_SYMMETRIC): 1 = the plane solve composes its step with symm_step_matrix; set when the loop starts
    int32_t pad4;
};

// Squared local search radius for the query p (rounded up to float).  Derivation: the pair test measures
// |mx2 a - mx2 b| in float32; for real local distance D the real world distance is >= sigma_min(mx2) D, and the
// float32 evaluation of the two products, the difference and the length is off by < 64u (|mx2|_inf (|a|+|b|) + |t|).
// init_loop_state() folds thresh, sigma_min, the target's extent and those error terms into cut_a, cut_b (+1e-5).
__host__ __device__ inline float search_cutoff2(const DevState *st, float px, float py, float pz)
{
    if (!(st->cut_a < 1e300)) return INFINITY;
    const double pabs = fabs((double)px) + fabs((double)py) + fabs((double)pz);
    const double c = st->cut_a + st->cut_b * pabs;
    const double c2 = c * c * (1.0 + 1e-6);
    return c2 < 3.0e38 ? (float)c2 : INFINITY;
}

// ------------------------------------------------------------------------------------------------
// float32 "mathutils" arithmetic (host + device, identical bits)
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline void m4_mul_v3(const float *M, float x, float y, float z, float &ox, float &oy, float &oz)
{
    // per row: double accumulation of float products, w = 1  (mathutils column_vector_multiplication)
    float r[3];
    for (int row = 0; row < 3; ++row) {
        const float *m = M + 4 * row;
        float p0 = m[0] * x, p1 = m[1] * y, p2 = m[2] * z, p3 = m[3] * 1.0f;
        double acc = 0.0;
        acc += (double)p0; acc += (double)p1; acc += (double)p2; acc += (double)p3;
        r[row] = (float)acc;
    }
    ox = r[0]; oy = r[1]; oz = r[2];
}

// co_find = imx2 @ (mx1 @ p)  (functions/general.py:287), the query of every search.  With the identity as the base object's
// matrix (DevState::mx2_identity; its inverse is then the identity too) the second product returns its argument bit for bit
// -- up to the sign of a zero, which no distance, cell or pair can see; a non-finite coordinate fails the searches' finiteness
// tests either way -- and is skipped: 39 fp32/fp64 instructions per query.
__host__ __device__ inline void co_find(const DevState *__restrict__ st, float x, float y, float z, float &px, float &py, float &pz)
{
    float wx, wy, wz;
    m4_mul_v3(st->mx1, x, y, z, wx, wy, wz);                       // mx1 @ p
    if (st->mx2_identity) { px = wx; py = wy; pz = wz; return; }
    m4_mul_v3(st->imx2, wx, wy, wz, px, py, pz);
}

__host__ __device__ inline void m4_mul_m4(const float *A, const float *B, float *out)
{
    float r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 4; ++k) { float p = A[4 * i + k] * B[4 * k + j]; acc += (double)p; }
            r[4 * i + j] = (float)acc;
        }
    for (int i = 0; i < 16; ++i) out[i] = r[i];
}

__host__ __device__ inline double v3_length(float x, float y, float z)
{
    double acc = 0.0;
    float pz = z * z, py = y * y, px = x * x;
    acc += (double)pz; acc += (double)py; acc += (double)px;   // last component first (mathutils dot_vn_vn)
    return sqrt(acc);
}

// Matrix.inverted() as Blender 3.2 computes it (mathutils_Matrix.c: matrix_invert_internal -> determinant_m4, adjoint_m4_m4,
// element / det; blenlib math_matrix.c), ALL in float, left to right, no fused multiply-add (this translation unit is compiled
// with -ffp-contract=off): bit-identical to oracle/oa_oracle.c: oo_mat4_inverted, which cites the routines.  mathutils stores a
// matrix column-major; m[i][j] below is Blender's matrix[i][j] = element (row j, column i) of the row-major argument, so the
// operand order inside every cofactor is Blender's.  false if the float determinant is exactly 0 (Blender raises ValueError).
__host__ __device__ inline float bl_det_m2(float a, float b, float c, float d) { return a * d - b * c; }
__host__ __device__ inline float bl_det_m3(float a1, float a2, float a3, float b1, float b2, float b3, float c1, float c2, float c3)
{
    return (a1 * bl_det_m2(b2, b3, c2, c3) - b1 * bl_det_m2(a2, a3, c2, c3)) + c1 * bl_det_m2(a2, a3, b2, b3);
}
// adjoint_m4_m4 + determinant_m4: R[i * 4 + j] = Blender's R[i][j]
__host__ __device__ inline void m4_adjoint_det(const float *Af, float R[16], float &det)
{
    const float a1 = Af[0], b1 = Af[4], c1 = Af[8], d1 = Af[12];    // m[0][0..3]: column 0
    const float a2 = Af[1], b2 = Af[5], c2 = Af[9], d2 = Af[13];
    const float a3 = Af[2], b3 = Af[6], c3 = Af[10], d3 = Af[14];
    const float a4 = Af[3], b4 = Af[7], c4 = Af[11], d4 = Af[15];
    det = (((a1 * bl_det_m3(b2, b3, b4, c2, c3, c4, d2, d3, d4) - b1 * bl_det_m3(a2, a3, a4, c2, c3, c4, d2, d3, d4)) +
            c1 * bl_det_m3(a2, a3, a4, b2, b3, b4, d2, d3, d4)) - d1 * bl_det_m3(a2, a3, a4, b2, b3, b4, c2, c3, c4));
    R[0]  = bl_det_m3(b2, b3, b4, c2, c3, c4, d2, d3, d4);
    R[4]  = -bl_det_m3(a2, a3, a4, c2, c3, c4, d2, d3, d4);
    R[8]  = bl_det_m3(a2, a3, a4, b2, b3, b4, d2, d3, d4);
    R[12] = -bl_det_m3(a2, a3, a4, b2, b3, b4, c2, c3, c4);
    R[1]  = -bl_det_m3(b1, b3, b4, c1, c3, c4, d1, d3, d4);
    R[5]  = bl_det_m3(a1, a3, a4, c1, c3, c4, d1, d3, d4);
    R[9]  = -bl_det_m3(a1, a3, a4, b1, b3, b4, d1, d3, d4);
    R[13] = bl_det_m3(a1, a3, a4, b1, b3, b4, c1, c3, c4);
    R[2]  = bl_det_m3(b1, b2, b4, c1, c2, c4, d1, d2, d4);
    R[6]  = -bl_det_m3(a1, a2, a4, c1, c2, c4, d1, d2, d4);
    R[10] = bl_det_m3(a1, a2, a4, b1, b2, b4, d1, d2, d4);
    R[14] = -bl_det_m3(a1, a2, a4, b1, b2, b4, c1, c2, c4);
    R[3]  = -bl_det_m3(b1, b2, b3, c1, c2, c3, d1, d2, d3);
    R[7]  = bl_det_m3(a1, a2, a3, c1, c2, c3, d1, d2, d3);
    R[11] = -bl_det_m3(a1, a2, a3, b1, b2, b3, d1, d2, d3);
    R[15] = bl_det_m3(a1, a2, a3, b1, b2, b3, c1, c2, c3);
}
__host__ __device__ inline bool m4_inverted(const float *Af, float *out)
{
    float R[16], det;
    m4_adjoint_det(Af, R, det);
    if (det == 0.0f) return false;
    // out (row-major) [j * 4 + i] = R[i][j] / det
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) out[j * 4 + i] = R[i * 4 + j] / det;
    return true;
}

// ------------------------------------------------------------------------------------------------
// 3x3 rotation from the covariance H = sum b a^T (Kabsch; functions/general.py:181-187).
// One-sided Jacobi gives H V = U S; the reflection-corrected rotation U diag(1,1,det(UV^T)) V^T equals
// [u1 u2 u1xu2][v1 v2 v1xv2]^T, so only the two leading singular triplets are needed (rank >= 2).
// ------------------------------------------------------------------------------------------------
// One Jacobi rotation of columns (P, Q) of g and v; returns whether the pair needed one.  P, Q are template
// parameters so that every index is static: on the device the arrays then live in registers instead of scratch
// memory (the solve is a single fp64 lane; a scratch round trip per element dominated it).
template <int P, int Q>
__host__ __device__ inline bool jacobi_rotate(double g[3][3], double v[3][3])
{
    const double npp = g[0][P] * g[0][P] + g[1][P] * g[1][P] + g[2][P] * g[2][P];
    const double nqq = g[0][Q] * g[0][Q] + g[1][Q] * g[1][Q] + g[2][Q] * g[2][Q];
    const double dpq = g[0][P] * g[0][Q] + g[1][P] * g[1][Q] + g[2][P] * g[2][Q];
    if (dpq == 0.0 || dpq * dpq <= 1e-30 * (npp * nqq)) return false;     // |dpq| <= 1e-15 |g_p||g_q| (~4.5 eps)
    // t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), zeta = (nqq - npp) / (2 dpq), written with one division:
    // t = 2 dpq sign(w) / (|w| + sqrt(w^2 + 4 dpq^2)), w = nqq - npp
    const double w = nqq - npp, d2 = 2.0 * dpq;
    double c, s;
#if defined(__HIP_DEVICE_COMPILE__)
    // On the device a rotation is a chain of dependent fp64 operations on ONE lane, and the IEEE sqrt and division
    // sequences were four fifths of it (~0.5 us per rotation, 8 rotations per solve: tools/solve_microbench.hip).  The
    // ANGLE only steers the convergence -- any (c, s) with c^2 + s^2 = 1 is an exact orthogonal update of g and v -- so
    // t comes from the hardware's reciprocal-square-root / reciprocal seeds plus one Newton step each (relative error
    // ~1e-13: the off-diagonal term this rotation is meant to cancel survives at that level and the next sweep's test
    // sees it far below its threshold), and c = (1 + t^2)^(-1/2) from the seed plus two Newton steps (full precision,
    // so that c^2 + s^2 = 1 to the last bits).  Out-of-range magnitudes take the IEEE formulas below.
    const double h2 = __builtin_fma(w, w, d2 * d2);
    if (h2 > 1e-280 && h2 < 1e280) {
        const double y = __builtin_amdgcn_rsq(h2);
        double hyp = h2 * y;
        hyp = __builtin_fma(0.5 * y, __builtin_fma(-hyp, hyp, h2), hyp);
        const double den = fabs(w) + hyp;
        double r = __builtin_amdgcn_rcp(den);
        r = __builtin_fma(r, __builtin_fma(-den, r, 1.0), r);
        const double t = (w >= 0.0 ? d2 : -d2) * r;
        const double q = __builtin_fma(t, t, 1.0);
        c = __builtin_amdgcn_rsq(q);
        c = c * __builtin_fma(-0.5 * q * c, c, 1.5);
        c = c * __builtin_fma(-0.5 * q * c, c, 1.5);
        s = c * t;
    } else
#endif
    {
        const double t = (w >= 0.0 ? d2 : -d2) / (fabs(w) + sqrt(w * w + d2 * d2));
        c = 1.0 / sqrt(1.0 + t * t);
        s = c * t;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 3; ++r) {
        const double gp = g[r][P], gq = g[r][Q], vp = v[r][P], vq = v[r][Q];
        g[r][P] = c * gp - s * gq; g[r][Q] = s * gp + c * gq;
        v[r][P] = c * vp - s * vq; v[r][Q] = s * vp + c * vq;
    }
    return true;
}

// column j of a 3x3 held in registers (select chain instead of a dynamic index)
__host__ __device__ inline double col3(const double m[3][3], int r, int j)
{
    return j == 0 ? m[r][0] : (j == 1 ? m[r][1] : m[r][2]);
}

// v_io (optional, 9 doubles, row-major): in = an orthogonal matrix to start from (the V of a similar covariance: then
// g = H V has nearly orthogonal columns already), out = the V this solve ends with.  Any orthogonal start gives the same
// singular vectors up to rounding.
__host__ __device__ inline void rotation_from_covariance(const double H[9], double R[9], double *v_io = nullptr, bool v_valid = false)
{
    double g[3][3], v[3][3];
    if (v_io && v_valid) {
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) v[i][j] = v_io[3 * i + j];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) g[i][j] = (H[3 * i] * v[0][j] + H[3 * i + 1] * v[1][j]) + H[3 * i + 2] * v[2][j];
    } else {
        g[0][0] = H[0]; g[0][1] = H[1]; g[0][2] = H[2];
        g[1][0] = H[3]; g[1][1] = H[4]; g[1][2] = H[5];
        g[2][0] = H[6]; g[2][1] = H[7]; g[2][2] = H[8];
        v[0][0] = 1.0; v[0][1] = 0.0; v[0][2] = 0.0;
        v[1][0] = 0.0; v[1][1] = 1.0; v[1][2] = 0.0;
        v[2][0] = 0.0; v[2][1] = 0.0; v[2][2] = 1.0;
    }
    for (int sweep = 0; sweep < 64; ++sweep) {
        bool any = jacobi_rotate<0, 1>(g, v);
        any = jacobi_rotate<0, 2>(g, v) || any;
        any = jacobi_rotate<1, 2>(g, v) || any;
        if (!any) break;
    }
    if (v_io)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) v_io[3 * i + j] = v[i][j];
    const double sg0 = sqrt(g[0][0] * g[0][0] + g[1][0] * g[1][0] + g[2][0] * g[2][0]);
    const double sg1 = sqrt(g[0][1] * g[0][1] + g[1][1] * g[1][1] + g[2][1] * g[2][1]);
    const double sg2 = sqrt(g[0][2] * g[0][2] + g[1][2] * g[1][2] + g[2][2] * g[2][2]);
    int j1 = 0;
    if (sg1 > sg0) j1 = 1;
    if (sg2 > (j1 == 0 ? sg0 : sg1)) j1 = 2;
    int j2 = (j1 == 0) ? 1 : 0;
    for (int j = 0; j < 3; ++j) {
        const double sj = j == 0 ? sg0 : (j == 1 ? sg1 : sg2), s2 = j2 == 0 ? sg0 : (j2 == 1 ? sg1 : sg2);
        if (j != j1 && sj > s2) j2 = j;
    }
    const double s_j1 = j1 == 0 ? sg0 : (j1 == 1 ? sg1 : sg2), s_j2 = j2 == 0 ? sg0 : (j2 == 1 ? sg1 : sg2);
    double u1[3], u2[3], v1[3], v2[3];
    const double i_j1 = (s_j1 > 0.0) ? 1.0 / s_j1 : 0.0, i_j2 = (s_j2 > 0.0) ? 1.0 / s_j2 : 0.0;   // (side by side: independent)
    for (int r = 0; r < 3; ++r) {
        v1[r] = col3(v, r, j1); v2[r] = col3(v, r, j2);
        u1[r] = (s_j1 > 0.0) ? col3(g, r, j1) * i_j1 : (r == 0 ? 1.0 : 0.0);
        u2[r] = (s_j2 > 0.0) ? col3(g, r, j2) * i_j2 : 0.0;
    }
    if (!(s_j2 > 0.0)) {   // rank <= 1: the rotation is not unique; complete u2 deterministically
        int m = 0;
        if (fabs(u1[1]) < fabs(u1[m])) m = 1;
        if (fabs(u1[2]) < fabs(m == 0 ? u1[0] : u1[1])) m = 2;
        const double e[3] = { m == 0 ? 1.0 : 0.0, m == 1 ? 1.0 : 0.0, m == 2 ? 1.0 : 0.0 };
        const double d = e[0] * u1[0] + e[1] * u1[1] + e[2] * u1[2];
        double nn = 0.0;
        for (int r = 0; r < 3; ++r) { u2[r] = e[r] - d * u1[r]; nn += u2[r] * u2[r]; }
        nn = sqrt(nn);
        for (int r = 0; r < 3; ++r) u2[r] /= nn;
    }
    const double u3[3] = { u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0] };
    const double v3[3] = { v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0] };
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = u1[i] * v1[j] + u2[i] * v2[j] + u3[i] * v3[j];
}

// Solve from the accumulated sums.  Returns false when K < 3 (the reference's ValueError).
// Horn's closed form (functions/general.py:191-206, usesvd=False): the rotation is the unit quaternion that is the eigenvector of
// the largest eigenvalue of the symmetric 4 x 4 matrix N built from the covariance (the reference hands N's lower triangle to
// numpy.linalg.eigh); here a cyclic Jacobi diagonalisation in fp64.  H[3 i + j] = sum v1_i v0_j, as rotation_from_covariance takes it.
__host__ __device__ inline void rotation_from_covariance_horn(const double H[9], double R[9])
{
    const double xx = H[0], yy = H[4], zz = H[8], xy = H[3], yz = H[7], zx = H[2], xz = H[6], yx = H[1], zy = H[5];
    double N[4][4] = { { xx + yy + zz, yz - zy, zx - xz, xy - yx },
                       { yz - zy, xx - yy - zz, xy + yx, zx + xz },
                       { zx - xz, xy + yx, yy - xx - zz, yz + zy },
                       { xy - yx, zx + xz, yz + zy, zz - xx - yy } };
    double V[4][4] = { { 1, 0, 0, 0 }, { 0, 1, 0, 0 }, { 0, 0, 1, 0 }, { 0, 0, 0, 1 } };
    for (int sweep = 0; sweep < 32; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < 4; ++p) { diag += fabs(N[p][p]); for (int q = p + 1; q < 4; ++q) off += fabs(N[p][q]); }
        if (!(off > 1e-300) || off <= 1e-18 * diag) break;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                if (N[p][q] == 0.0) continue;
                const double theta = (N[q][q] - N[p][p]) / (2.0 * N[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < 4; ++k) { const double a = N[k][p], b = N[k][q]; N[k][p] = c * a - sn * b; N[k][q] = sn * a + c * b; }
                for (int k = 0; k < 4; ++k) { const double a = N[p][k], b = N[q][k]; N[p][k] = c * a - sn * b; N[q][k] = sn * a + c * b; }
                for (int k = 0; k < 4; ++k) { const double a = V[k][p], b = V[k][q]; V[k][p] = c * a - sn * b; V[k][q] = sn * a + c * b; }
            }
    }
    int m = 0;
    for (int k = 1; k < 4; ++k) if (N[k][k] > N[m][m]) m = k;
    double q[4] = { V[0][m], V[1][m], V[2][m], V[3][m] };
    const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (!(n2 > 0.0)) { for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0; return; }
    const double f = sqrt(2.0 / n2);                                 // quaternion_matrix (:54-62): q *= sqrt(2 / n), then the outer products
    for (int k = 0; k < 4; ++k) q[k] *= f;
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0 - y * y - z * z; R[1] = x * y - z * w;       R[2] = x * z + y * w;
    R[3] = x * y + z * w;       R[4] = 1.0 - x * x - z * z; R[5] = y * z - x * w;
    R[6] = x * z - y * w;       R[7] = y * z + x * w;       R[8] = 1.0 - x * x - y * y;
}

// x -= a b / k for x = hi + lo held in two doubles.  The product, the quotient and the difference each keep their own rounding
// error (the fused multiply-adds return the exact remainders), so what is lost is a rounding of the RESULT, not of the operands.
__host__ __device__ inline void dd_sub_prod_quot(double &hi, double &lo, double a, double b, double k)
{
    const double p = a * b, pe = __builtin_fma(a, b, -p);
    const double q = p / k, qe = (__builtin_fma(-q, k, p) + pe) / k;
    const double s = hi - q, bb = s - hi;
    lo += ((hi - (s - bb)) - (q + bb)) - qe;
    hi = s;
}
// The centred moments below are differences of sums about the pivot: S_H - K c_b c_a^T, S_AA - K |c_a|^2.  With the pivot inside
// the cloud (every loop: the first source vertex) the two terms differ by a small factor and nothing is lost.  A pivot far from
// the cloud (oa_kabsch_from_sums about the origin, a cloud 3e4 away: the terms are 1e9 times the difference) loses that factor
// of the 53 bits -- 1e-7 in R where 1e-16 was due.  Where a difference is more than CANCEL_GATE times smaller than its first term
// it is redone in two doubles; below the gate (at most 6 bits lost) the plain result stands, bit for bit what it always was.
constexpr double CANCEL_GATE = 64.0;

// weighted: the sums [0..16] carry the pairs' weights and S_W their mass -- centroids, covariance and the scale branch are the
// weighted ones; the rule K >= 3 still counts pairs, and a mass that is not > 0 fails like it.
__host__ __device__ inline bool solve_from_sums(const double *s, const double pivot[3], bool with_scale, double M[16],
                                                double *v_io = nullptr, bool v_valid = false, bool horn = false, bool weighted = false)
{
    if (!(s[S_K] >= 3.0)) return false;
    const double K = weighted ? s[S_W] : s[S_K];
    if (!(K > 0.0)) return false;
    double ca[3], cb[3];
    const double inv_K = 1.0 / K;
    for (int i = 0; i < 3; ++i) { ca[i] = s[S_A + i] * inv_K; cb[i] = s[S_B + i] * inv_K; }     // centroids (:160,:164)
    double H[9], h_max = 0.0, s_max = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            H[3 * i + j] = s[S_H + 3 * i + j] - K * cb[i] * ca[j];                            // dot(v1c, v0c.T) (:181)
            h_max = fmax(h_max, fabs(H[3 * i + j])); s_max = fmax(s_max, fabs(s[S_H + 3 * i + j]));
        }
    if (s_max > CANCEL_GATE * h_max)                                                        // (false for NaN: the plain result stands)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double hi = s[S_H + 3 * i + j], lo = 0.0;
                dd_sub_prod_quot(hi, lo, s[S_B + i], s[S_A + j], K);
                H[3 * i + j] = hi + lo;
            }
    double R[9];
    if (horn) rotation_from_covariance_horn(H, R);                  // usesvd=False (:191-206)
    else rotation_from_covariance(H, R, v_io, v_valid);
    double sc = 1.0;
    if (with_scale) {                                                                    // :208-212
        double n0 = s[S_AA] - K * (ca[0] * ca[0] + ca[1] * ca[1] + ca[2] * ca[2]);
        double n1 = s[S_BB] - K * (cb[0] * cb[0] + cb[1] * cb[1] + cb[2] * cb[2]);
        if (s[S_AA] > CANCEL_GATE * fabs(n0)) {
            double hi = s[S_AA], lo = 0.0;
            for (int i = 0; i < 3; ++i) dd_sub_prod_quot(hi, lo, s[S_A + i], s[S_A + i], K);
            n0 = hi + lo;
        }
        if (s[S_BB] > CANCEL_GATE * fabs(n1)) {
            double hi = s[S_BB], lo = 0.0;
            for (int i = 0; i < 3; ++i) dd_sub_prod_quot(hi, lo, s[S_B + i], s[S_B + i], K);
            n1 = hi + lo;
        }
        sc = sqrt(n1 / n0);
    }
    // back to un-pivoted coordinates: c0 = ca + pivot, c1 = cb + pivot;  t = c1 - sR c0   (:215)
    for (int i = 0; i < 3; ++i) {
        double t = cb[i] + pivot[i];
        for (int j = 0; j < 3; ++j) {
            M[4 * i + j] = sc * R[3 * i + j];
            t -= sc * R[3 * i + j] * (ca[j] + pivot[j]);
        }
        M[4 * i + 3] = t;
    }
    M[12] = 0.0; M[13] = 0.0; M[14] = 0.0; M[15] = 1.0;
    return true;
}

__host__ __device__ inline double rotation_angle_3x3(const double M[16])
{
    // |angle| of the rotation part (columns normalised first, so uniform scale does not matter)
    double c[3];
    for (int j = 0; j < 3; ++j) c[j] = sqrt(M[j] * M[j] + M[4 + j] * M[4 + j] + M[8 + j] * M[8 + j]);
    double tr = 0.0;
    for (int j = 0; j < 3; ++j) tr += (c[j] > 0.0) ? M[4 * j + j] / c[j] : 1.0;
    double x = (tr - 1.0) * 0.5;
    x = x > 1.0 ? 1.0 : (x < -1.0 ? -1.0 : x);
    return acos(x);
}

// ------------------------------------------------------------------------------------------------
// The point-to-plane step from its sums: (sum J J^T) x = -sum J r, minimum-norm solution through the symmetric
// eigen-decomposition (cyclic Jacobi in fp64, the pattern of rotation_from_covariance_horn), then M = T(c) T(t) R T(-c) with
// R = exp([omega]x) (Rodrigues: an exact rotation, so the float32 matrix_world never picks up shear from the step).
// ------------------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
#define OA_WAVE_LDS_FENCE() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront")
#else
#define OA_WAVE_LDS_FENCE() ((void)0)
#endif

// position of (i, j), i <= j, in the upper triangle stored by rows
__host__ __device__ inline int sym6_index(int i, int j) { return 6 * i - (i * (i - 1)) / 2 + (j - i); }

// Eigen-decomposition of the symmetric 6 x 6 in A (row-major, 36 doubles): on return its diagonal holds the eigenvalues and the
// columns of V the eigenvectors.  Written for ONE WAVEFRONT with A and V in LDS (dynamic indices, no registers spent on 72
// doubles): every lane computes a rotation's angle from the same three entries, lane k in [k0, k1) applies it to row / column k.
// The device passes k0 = lane, k1 = lane + 1 for lanes 0..5 and an empty range for the others; a single thread (the host)
// passes [0, 6) and runs the same arithmetic serially.  Called by all lanes of the wave.
__host__ __device__ inline void sym6_jacobi(double *A, double *V, int k0, int k1)
{
    for (int k = k0; k < k1; ++k)
        for (int j = 0; j < 6; ++j) V[6 * k + j] = (j == k) ? 1.0 : 0.0;
    OA_WAVE_LDS_FENCE();
    for (int sweep = 0; sweep < 32; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < 6; ++p) { diag += fabs(A[7 * p]); for (int q = p + 1; q < 6; ++q) off += fabs(A[6 * p + q]); }
        if (!(off > 1e-300) || off <= 1e-18 * diag) break;
        for (int p = 0; p < 5; ++p)
            for (int q = p + 1; q < 6; ++q) {
                const double apq = A[6 * p + q], app = A[7 * p], aqq = A[7 * q];
                if (apq == 0.0) continue;                                   // (uniform: every lane reads the same entry)
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                OA_WAVE_LDS_FENCE();                                        // the reads above, before any lane's writes below
                for (int k = k0; k < k1; ++k) {                             // columns p, q of A and of V
                    const double a = A[6 * k + p], b = A[6 * k + q]; A[6 * k + p] = c * a - sn * b; A[6 * k + q] = sn * a + c * b;
                    const double u = V[6 * k + p], w = V[6 * k + q]; V[6 * k + p] = c * u - sn * w; V[6 * k + q] = sn * u + c * w;
                }
                OA_WAVE_LDS_FENCE();
                for (int k = k0; k < k1; ++k) {                             // rows p, q of A
                    const double a = A[6 * p + k], b = A[6 * q + k]; A[6 * p + k] = c * a - sn * b; A[6 * q + k] = sn * a + c * b;
                }
                OA_WAVE_LDS_FENCE();
            }
    }
}

// Eigenvalues below PLANE_EIG_CUT x the largest count as zero: a plane, a sphere, a cylinder leave 3 / 3 / 2 directions of
// (omega, t) the data cannot see, and the step must not move along them.  A guard, not a tuning knob.
constexpr double PLANE_EIG_CUT = 1e-10;

// M = T(c) T(t) exp([omega]x) T(-c), x = (omega, t)
__host__ __device__ inline void plane_step_matrix(const double x[6], const double c[3], double M[16])
{
    const double wx = x[0], wy = x[1], wz = x[2];
    const double th2 = (wx * wx + wy * wy) + wz * wz;
    double a, b;                                                            // sin(th) / th, (1 - cos(th)) / th^2
    if (th2 < 1e-8) {                                                       // th < 1e-4: the series, next term th^6 / 5040
        a = 1.0 - th2 / 6.0 * (1.0 - th2 / 20.0);
        b = 0.5 - th2 / 24.0 * (1.0 - th2 / 30.0);
    } else {
        const double th = sqrt(th2), sh = sin(0.5 * th);
        a = sin(th) / th;
        b = 2.0 * sh * sh / th2;
    }
    const double d = 1.0 - b * th2;
    double R[9];
    R[0] = d + b * wx * wx;      R[1] = b * wx * wy - a * wz; R[2] = b * wx * wz + a * wy;
    R[3] = b * wx * wy + a * wz; R[4] = d + b * wy * wy;      R[5] = b * wy * wz - a * wx;
    R[6] = b * wx * wz - a * wy; R[7] = b * wy * wz + a * wx; R[8] = d + b * wz * wz;
    for (int i = 0; i < 3; ++i) {
        double t = c[i] + x[3 + i];
        for (int j = 0; j < 3; ++j) { M[4 * i + j] = R[3 * i + j]; t -= R[3 * i + j] * c[j]; }
        M[4 * i + 3] = t;
    }
    M[12] = 0.0; M[13] = 0.0; M[14] = 0.0; M[15] = 1.0;
}

// The symmetric metric's step (Rusinkiewicz 2019), x = (a~, t~) the solution of its linear system: the rotation is split between
// both sides, M = T(c) R T(t) R T(-c) with theta = atan(|a~|), R = exp(theta [a~ / |a~|]x), t = t~ cos(theta).  With K = [a~]x,
// R = I + a K + b K K, a = sin(theta) / |a~|, b = (1 - cos(theta)) / |a~|^2 -- both finite as |a~| -> 0 (1 and 1/2).
__host__ __device__ inline void symm_step_matrix(const double x[6], const double c[3], double M[16])
{
    const double wx = x[0], wy = x[1], wz = x[2];
    const double a2 = (wx * wx + wy * wy) + wz * wz;
    double ct, a, b;                                                        // cos(theta), sin(theta) / |a~|, (1 - cos(theta)) / |a~|^2
    if (a2 < 1e-8) {                                                        // |a~| < 1e-4: the series in |a~|^2, next term |a~|^6
        ct = 1.0 - a2 / 2.0 * (1.0 - a2 * 0.75);
        a = ct;                                                             // (sin(atan u) / u = cos(atan u))
        b = 0.5 - a2 * 0.375 * (1.0 - a2 / 1.2);
    } else {
        const double u = sqrt(a2), th = atan(u), sh = sin(0.5 * th);
        ct = cos(th);
        a = sin(th) / u;
        b = 2.0 * sh * sh / a2;
    }
    const double d = 1.0 - b * a2;
    double R[9], t[3], Rt[3];
    R[0] = d + b * wx * wx;      R[1] = b * wx * wy - a * wz; R[2] = b * wx * wz + a * wy;
    R[3] = b * wx * wy + a * wz; R[4] = d + b * wy * wy;      R[5] = b * wy * wz - a * wx;
    R[6] = b * wx * wz - a * wy; R[7] = b * wy * wz + a * wx; R[8] = d + b * wz * wz;
    for (int i = 0; i < 3; ++i) t[i] = x[3 + i] * ct;
    for (int i = 0; i < 3; ++i) Rt[i] = (R[3 * i] * t[0] + R[3 * i + 1] * t[1]) + R[3 * i + 2] * t[2];
    for (int i = 0; i < 3; ++i) {                                           // M v = c + R (t + R (v - c))
        double tr = c[i] + Rt[i];
        for (int j = 0; j < 3; ++j) {
            const double r2 = (R[3 * i] * R[j] + R[3 * i + 1] * R[3 + j]) + R[3 * i + 2] * R[6 + j];
            M[4 * i + j] = r2;
            tr -= r2 * c[j];
        }
        M[4 * i + 3] = tr;
    }
    M[12] = 0.0; M[13] = 0.0; M[14] = 0.0; M[15] = 1.0;
}

// s: the NSUMS_PLANE sums (readable by every caller); A, V: 36 doubles of workspace each, shared by the callers (LDS on the
// device); [k0, k1): see sym6_jacobi.  Returns false when K < 3 (OA_E_TOO_FEW_PAIRS, as the point metric); rank = the
// eigenvalues kept (6 = the pairs determine the whole step).  Called by all lanes of one wave / by one host thread.
// symmetric: the sums are the symmetric metric's (symm_row) and x composes through symm_step_matrix.
__host__ __device__ inline bool plane_solve_from_sums(const double *s, const double pivot[3], double *A, double *V, int k0, int k1,
                                                      double M[16], int &rank, bool weighted = false, bool symmetric = false)
{
    rank = 0;
    if (!(s[P_K] >= 3.0)) return false;
    if (weighted && !(s[P_W] > 0.0)) return false;                          // (weighted rows: a mass that is not > 0 fails like K < 3)
    for (int k = k0; k < k1; ++k)
        for (int j = 0; j < 6; ++j) A[6 * k + j] = s[P_JJ + (k <= j ? sym6_index(k, j) : sym6_index(j, k))];
    OA_WAVE_LDS_FENCE();
    sym6_jacobi(A, V, k0, k1);
    double lam_max = 0.0;
    for (int i = 0; i < 6; ++i) lam_max = A[7 * i] > lam_max ? A[7 * i] : lam_max;
    const double cut = PLANE_EIG_CUT * lam_max;
    double x[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double lam = A[7 * i];
        if (!(lam > cut) || !(lam > 0.0)) continue;
        ++rank;
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) d += V[6 * k + i] * s[P_JR + k];
        const double f = -d / lam;
#pragma unroll
        for (int j = 0; j < 6; ++j) x[j] += f * V[6 * j + i];
    }
    if (symmetric) symm_step_matrix(x, pivot, M); else plane_step_matrix(x, pivot, M);
    return true;
}

// ------------------------------------------------------------------------------------------------
// closest point on a triangle (surface mode, oa_tri.hpp): Blender's closest_on_tri_to_point_v3 restated in float32
// with explicit operation order and no fma; bit-identical to oracle/oa_oracle.c: oo_closest_on_tri
// ------------------------------------------------------------------------------------------------
__host__ __device__ inline float dot3f(const float *a, const float *b)
{
    float s = a[0] * b[0];
    s = s + a[1] * b[1];
    s = s + a[2] * b[2];
    return s;
}

// Blender math_geom.c closest_on_tri_to_point_v3, float32: the oracle's operations on the oracle's operands, but WITHOUT its
// early returns.  A wavefront takes every branch some lane takes, and with seven ways out (three vertices, three edges, the
// inside) the branchy form cost 370 instructions per call, the tail behind each return included.  Here everything the regions
// need is computed once (six dot products, the three cross terms), the region is the first of the oracle's tests that holds,
// ONE division serves whichever region it is (its numerator and denominator are selected first: the same IEEE quotient of
// the same two floats), and the point is put together from selected operands: ~150 instructions, the same bits.
// (A region's own expressions are evaluated for lanes outside it too; what they produce there -- a 0 / 0, say -- is dropped.)
__host__ __device__ inline void closest_on_tri(const float *p, const float *a, const float *b, const float *c, float *r)
{
    // (scalars, not arrays: selects between array elements keep the arrays in scratch memory)
    const float ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2], cx = c[0], cy = c[1], cz = c[2];
    const float px = p[0], py = p[1], pz = p[2];
    const float abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
    const float apx = px - ax, apy = py - ay, apz = pz - az, bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const float cpx = px - cx, cpy = py - cy, cpz = pz - cz, cbx = cx - bx, cby = cy - by, cbz = cz - bz;
#define OA_DOT3(ux, uy, uz, vx, vy, vz) (((ux) * (vx) + (uy) * (vy)) + (uz) * (vz))          /* dot3f's order */
    const float d1 = OA_DOT3(abx, aby, abz, apx, apy, apz), d2 = OA_DOT3(acx, acy, acz, apx, apy, apz);
    const float d3 = OA_DOT3(abx, aby, abz, bpx, bpy, bpz), d4 = OA_DOT3(acx, acy, acz, bpx, bpy, bpz);
    const float d5 = OA_DOT3(abx, aby, abz, cpx, cpy, cpz), d6 = OA_DOT3(acx, acy, acz, cpx, cpy, cpz);
#undef OA_DOT3
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float d43 = d4 - d3, d56 = d5 - d6;
    // the oracle's tests, in the oracle's order: the first that holds names the region
    const bool at_a = d1 <= 0.0f && d2 <= 0.0f;
    const bool at_b = d3 >= 0.0f && d4 <= d3;
    const bool on_ab = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
    const bool at_c = d6 >= 0.0f && d5 <= d6;
    const bool on_ac = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
    const bool on_bc = va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f;
    enum { AT_A, AT_B, ON_AB, AT_C, ON_AC, ON_BC, INSIDE };
    const int region = at_a ? AT_A : at_b ? AT_B : on_ab ? ON_AB : at_c ? AT_C : on_ac ? ON_AC : on_bc ? ON_BC : INSIDE;
    // the one quotient: d1 / (d1 - d3) on ab, d2 / (d2 - d6) on ac, (d4 - d3) / ((d4 - d3) + (d5 - d6)) on bc,
    // 1 / ((va + vb) + vc) inside
    const float num = region == ON_AB ? d1 : region == ON_AC ? d2 : region == ON_BC ? d43 : 1.0f;
    const float den = region == ON_AB ? d1 - d3 : region == ON_AC ? d2 - d6 : region == ON_BC ? d43 + d56 : (va + vb) + vc;
    const float q = num / den;
    const float s1 = region == INSIDE ? vb * q : q;                // inside: v = vb * denom
    const float s2 = vc * q;                                       //         w = vc * denom
    const bool from_b = region == ON_BC || region == AT_B, from_c = region == AT_C;
    const bool vertex = region == AT_A || region == AT_B || region == AT_C, inside = region == INSIDE;
    const bool along_ac = region == ON_AC, along_cb = region == ON_BC;
    // t: a + ab v | a + ac w | (c - b) w + b | a + ab v;   inside: t + ac w
#define OA_TRI_POINT(k, av, bv, cv, abv, acv, cbv)                                                       \
    {                                                                                                    \
        const float base = from_b ? (bv) : (from_c ? (cv) : (av));                                       \
        const float e1 = along_ac ? (acv) : (along_cb ? (cbv) : (abv));                                  \
        const float t = base + e1 * s1;                                                                  \
        const float in = t + (acv) * s2;                                                                 \
        r[k] = vertex ? base : (inside ? in : t);                                                        \
    }
    OA_TRI_POINT(0, ax, bx, cx, abx, acx, cbx)
    OA_TRI_POINT(1, ay, by, cy, aby, acy, cby)
    OA_TRI_POINT(2, az, bz, cz, abz, acz, cbz)
#undef OA_TRI_POINT
}

__host__ __device__ inline float tri_dist2(const float *p, const float *r)
{
    const float d[3] = { r[0] - p[0], r[1] - p[1], r[2] - p[2] };
    return dot3f(d, d);
}


#if defined(__HIPCC__)

// triangle image: 3 x float4 per triangle {ax,ay,az,bx} {by,bz,cx,cy} {cz,-,-,-}
__device__ __forceinline__ void load_tri(const float4 *__restrict__ tri9, long long t, float *a, float *b, float *c)
{
    const float4 u = tri9[3 * t], v = tri9[3 * t + 1], w = tri9[3 * t + 2];
    a[0] = u.x; a[1] = u.y; a[2] = u.z; b[0] = u.w; b[1] = v.x; b[2] = v.y; c[0] = v.z; c[1] = v.w; c[2] = w.x;
}

// ------------------------------------------------------------------------------------------------
// packing kernels (one-time)
// ------------------------------------------------------------------------------------------------
// source: gather xyz[vlist[(begin + i) * stride]] -> float4; the tail up to ns_pad repeats the last point
#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
__global__ void k_pack_source(const float *__restrict__ xyz, const long long *__restrict__ vlist, long long stride,
                              long long begin, const int *__restrict__ members, int ns, int ns_pad,
                              float4 *__restrict__ src4, int *__restrict__ sel_vertex)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns_pad) return;
    const int k = i < ns ? i : (ns > 0 ? ns - 1 : 0);
    const long long s = members ? (long long)members[k] : begin + (long long)k;   // position in the selection
    const long long v = vlist ? vlist[s * stride] : s * stride;
    float4 p;
    p.x = xyz[3 * v]; p.y = xyz[3 * v + 1]; p.z = xyz[3 * v + 2]; p.w = 0.f;
    src4[i] = p;
    sel_vertex[i] = (int)v;                       // which vertex this slot holds (normals are gathered with it)
}

__global__ void k_gather_rows3(const float *__restrict__ rows, const int *__restrict__ sel, int n, float *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long v = sel[i];
    out[3ll * i] = rows[3 * v]; out[3ll * i + 1] = rows[3 * v + 1]; out[3ll * i + 2] = rows[3 * v + 2];
}
// the same for one value per vertex (oa_set_source_weights)
__global__ void k_gather_rows1(const float *__restrict__ vals, const int *__restrict__ sel, int n, float *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = vals[(long long)sel[i]];
}
#endif  // !OA_FAMILY_TU

// 30-bit Morton key of a source point inside the source bounding box (spatial sort of the source slots: lanes of a
// wave then work on neighbouring points, which turns the grid search's scattered reads into mostly shared lines)
__device__ __forceinline__ unsigned spread10(unsigned v)
{
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
__global__ void k_morton_keys(const float4 *__restrict__ src4, int ns, float lx, float ly, float lz, float sx, float sy,
                              float sz, unsigned *__restrict__ keys)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const float4 p = src4[i];
    const float fx = fminf(fmaxf((p.x - lx) * sx, 0.f), 1023.f), fy = fminf(fmaxf((p.y - ly) * sy, 0.f), 1023.f),
                fz = fminf(fmaxf((p.z - lz) * sz, 0.f), 1023.f);      // NaN -> 0 through fmaxf
    keys[i] = spread10((unsigned)fx) | (spread10((unsigned)fy) << 1) | (spread10((unsigned)fz) << 2);
}

// sorted slot i takes original slot perm[i]; the padding repeats the last sorted point
__global__ void k_apply_perm(const float4 *__restrict__ src4o, const int *__restrict__ selo, const int *__restrict__ perm,
                             int ns, int ns_pad, float4 *__restrict__ src4, int *__restrict__ sel)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns_pad) return;
    const int o = perm[i < ns ? i : (ns > 0 ? ns - 1 : 0)];
    src4[i] = src4o[o];
    sel[i] = selo[o];
}

__global__ void k_iota(int *__restrict__ a, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = i;
}

// A shard adopted from the whole-selection order (oa_icp.hip: adopt_shard): src4 / sel hold its n points in slot
// (Morton) order; inv[m] = the slot of the shard's m-th point in the caller's order.  Fills the caller-order copy and the
// slot -> caller-order permutation, and pads both images to ns_pad by repeating their last point -- the layout
// k_pack_source + k_apply_perm leave behind.
__global__ void k_finish_shard(const int *__restrict__ inv, int n, int ns_pad, float4 *__restrict__ src4, int *__restrict__ sel,
                               float4 *__restrict__ src4o, int *__restrict__ perm)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns_pad) return;
    const int m = i < n ? i : n - 1;
    const int s = inv[m];
    src4o[i] = src4[s];
    if (i < n) perm[s] = i;
    else { src4[i] = src4[n - 1]; sel[i] = sel[n - 1]; }
}

// target: groups of 4 vertices as [x0..x3][y0..y3][z0..z3]; vertices past nt are +INF (never selected)
__global__ void k_pack_target(const float *__restrict__ xyz, int nt, int n_groups_pad, float4 *__restrict__ tg)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups_pad) return;
    float c[3][4];
    for (int k = 0; k < 4; ++k) {
        const long long v = 4ll * g + k;
        for (int a = 0; a < 3; ++a) c[a][k] = (v < nt) ? xyz[3 * v + a] : INFINITY;
    }
    for (int a = 0; a < 3; ++a) tg[3 * (long long)g + a] = make_float4(c[a][0], c[a][1], c[a][2], c[a][3]);
}

__global__ void k_fill_keys(unsigned long long *keys, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = KEY_EMPTY;
}

// everything a shard's slots start from, in ONE launch (it was six operations -- four memsets and two fills -- and an upload
// is bound by the host's ~5 us per enqueued operation): no seed (prev = -1, win = all ones: index -1, wsafe = all ones),
// empty keys, sel = 0 and the hand-over counters at zero.  Null pointers are skipped (oa_reset_seeds, a new target: the
// seeds only).
__global__ void k_init_slots(int *__restrict__ prev, float4 *__restrict__ win, uint2 *__restrict__ wsafe,
                             unsigned long long *__restrict__ keys, int *__restrict__ sel, int *__restrict__ todo_count, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && todo_count) { todo_count[0] = 0; todo_count[1] = 0; }
    if (i >= n) return;
    const float ones = __uint_as_float(0xFFFFFFFFu);
    if (prev) prev[i] = -1;
    if (win) win[i] = make_float4(ones, ones, ones, ones);
    if (wsafe) wsafe[i] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
    if (keys) keys[i] = KEY_EMPTY;
    if (sel) sel[i] = 0;
}

__global__ void k_fill_int(int *a, int n, int v)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = v;
}

// (d2, idx) keys -> separate arrays (first n_out entries); resets all n keys for the next search
__global__ void k_decode_keys(unsigned long long *__restrict__ keys, int n, int n_out, const int *__restrict__ perm,
                              long long *__restrict__ idx, float *__restrict__ d2)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    keys[i] = KEY_EMPTY;
    if (i >= n_out) return;
    const int o = perm ? perm[i] : i;                 // outputs are in the caller's (vlist) order
    const uint32_t j = (uint32_t)key;
    if (idx) idx[o] = (j == IDX_NONE) ? -1ll : (long long)j;
    if (d2) d2[o] = __uint_as_float((uint32_t)(key >> 32));
}
#endif  // !OA_FAMILY_TU

// ------------------------------------------------------------------------------------------------
// k_nn_search
// ------------------------------------------------------------------------------------------------
// grid = (n_splits, ns_pad / (256*R)): the split index is the FAST grid dimension, so with n_splits a multiple of 8
// the dispatcher's block -> XCD round-robin (block b on XCD b % 8) pins each target split to one XCD and that XCD's
// 4 MiB L2 keeps its 1/8 of the target image resident for the whole launch.  Each thread owns R source points (registers); the workgroup streams its
// split of the target through a double-buffered LDS tile.  All 64 lanes of a wave read the SAME LDS address
// (broadcast, conflict-free), so one ds_read_b128 feeds 4 targets x R points x 64 lanes = 256 R pair evaluations.
//
// Per group of 4 targets and per point: 4 x (3 sub, 1 mul, 2 fma) + 2 min3 + 1 compare = 27 VALU ops; the index
// is only resolved inside the (rare, exec-masked) `improved` branch.  Strict `<` against the running best and a
// lowest-k scan inside the group give "lowest index wins ties" exactly as the oracle's linear scan does.
__device__ __forceinline__ float d2_metric(float px, float py, float pz, float qx, float qy, float qz)
{
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    float t = dx * dx;
    t = __builtin_fmaf(dy, dy, t);
    t = __builtin_fmaf(dz, dz, t);
    return t;
}

// XCD-aware workgroup order for the one-thread-per-query searches.  The dispatcher deals workgroups out round-robin -- workgroup
// b runs on XCD b % 8 -- so with the plain order every XCD's L2 sees every eighth workgroup of the whole (Morton-ordered)
// query range: neighbours in space, which read the same cells, sit on eight different L2s.  With this order XCD x works
// through ONE contiguous eighth of the query range: virtual index = start(x) + b / 8, start(x) = x q + min(x, r) for
// gridDim.x = 8 q + r (a bijection of 0 .. gridDim.x - 1).  Everything a workgroup does -- its queries, its row of
// partials -- goes by the virtual index, so results are unchanged.  Measured (A/B, two rounds each): 1M <-> 1M 60.3 -> 59.5 us per
// iteration, the surface search (1M points, 1.96M triangles) 0.630 -> 0.615 ms settled, nothing in its cold regime; shards of
// fewer than 1024 workgroups lose a little (100k: 29.8 -> 30.7 us) and keep the plain order.
__device__ __forceinline__ int xcd_block_index()
{
    const int nb = (int)gridDim.x, b = (int)blockIdx.x;
    if (nb < 1024) return b;
    const int x = b & 7, q = nb >> 3, r = nb & 7;
    return x * q + (x < r ? x : r) + (b >> 3);
}

// The same in chunks (round 6, k_tri_search_grid while the pose still moves): an XCD's share of the launch is every eighth CHUNK of
// `chunk` consecutive workgroups instead of one contiguous eighth of them all.  The queries are in Morton order, their cost follows
// the geometry, and a contiguous eighth is one region of the object: on the first search of a cold start XCD 0's share took 825 us
// of slot time where the mean was 642, and the launch ended with it (1004 us; per-workgroup stamps, profiles/r06i) -- seven XCDs
// idle for a third of the launch.  Chunks hand every XCD the same mix of regions; once the pose has settled the contiguous share
// is the faster one again (neighbours read the same cell lists and triangles: 0.341 against 0.355 ms per search), so the search
// picks by the test its candidate budget already makes.  The last, partial round of chunks goes by the plain order.
__device__ __forceinline__ int xcd_block_index_chunked(int chunk)
{
    const int nb = (int)gridDim.x, b = (int)blockIdx.x;
    if (nb < 1024) return b;
    const int round = 8 * chunk, full = nb / round * round;         // workgroups in whole rounds of 8 chunks
    if (b >= full) return b;
    const int x = b & 7, k = b >> 3;                                // XCD, and this workgroup's number on it
    return (k / chunk) * round + x * chunk + k % chunk;
}

// "The pose still moves": first search of a loop, or last iteration's translation + rotation x object size above `threshold`
// (local units) -- the test behind the grid searches' budget_moving
__device__ __forceinline__ bool pose_moving(const DevState *__restrict__ st, double scale, double threshold)
{
    if (st->n == 0) return true;
    if (!st->use_target) return false;
    const int last = (st->n + 4) % 5;
    return (st->ring_t[last] + st->ring_r[last] * scale) * st->local_per_world > threshold;
}

// Target split of workgroup blockIdx.x: tiles [x T / n, (x + 1) T / n) of the T tiles (of `tile_groups` groups each), n =
// gridDim.x.  Split sizes differ by at most one tile, every split is non-empty (n <= T), and n stays what the host chose -- a
// multiple of 8 above 8, so that the dispatcher's round-robin (workgroup b on XCD b % 8) pins every split to ONE XCD, whose
// L2 then keeps its part of the image for the whole launch.  (Round 2 cut equal splits of ceil(T / n) tiles and launched
// ceil(T / that) of them: 70 instead of 72 for a 250k-point shard, 123 instead of 136 for 125k -- every XCD then saw every
// split, the 12 MB image no longer stayed in the L2s and the HBM-side traffic of a launch rose from 0.3 to 3.4 GB;
// profiles/r03d_bench_1Mx1M_pmc_summary.txt, the 4- and 8-shard passes.)
__device__ __forceinline__ void split_range(int n_groups_pad, int tile_groups, int &g_begin, int &g_end)
{
    const long long tiles = n_groups_pad / tile_groups;
    g_begin = (int)((long long)blockIdx.x * tiles / gridDim.x) * tile_groups;
    g_end = (int)((long long)(blockIdx.x + 1) * tiles / gridDim.x) * tile_groups;
}

__device__ __forceinline__ void split_range_of(int split, int n_splits, int n_groups_pad, int tile_groups, int &g_begin, int &g_end)
{
    const long long tiles = n_groups_pad / tile_groups;
    g_begin = (int)((long long)split * tiles / n_splits) * tile_groups;
    g_end = (int)((long long)(split + 1) * tiles / n_splits) * tile_groups;
}

template <int R>
__global__ __launch_bounds__(NN_THREADS) void k_nn_search(const DevState *__restrict__ st,
                                                          const float4 *__restrict__ src4,
                                                          const float4 *__restrict__ tg,
                                                          int n_groups_pad, unsigned long long *__restrict__ keys)
{
    if (st->halt) return;
    __shared__ float4 tile[2][TILE_GROUPS * 3];
    const int tid = threadIdx.x;
    const int base = blockIdx.y * (NN_THREADS * R);

    float px[R], py[R], pz[R], best[R];
    uint32_t bidx[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float4 p = src4[base + r * NN_THREADS + tid];
        co_find(st, p.x, p.y, p.z, px[r], py[r], pz[r]);    // imx2 @ (...) = co_find (general.py:287)
        best[r] = INFINITY;
        bidx[r] = IDX_NONE;
    }

    int g_begin, g_end;
    split_range(n_groups_pad, TILE_GROUPS, g_begin, g_end);
    const int n_tiles = (g_end - g_begin) / TILE_GROUPS;           // splits are whole tiles by construction
    const float4 *tsrc = tg + 3ll * g_begin;

    // prologue: tile 0
    float4 s0 = tsrc[tid], s1 = tsrc[NN_THREADS + tid], s2 = tsrc[2 * NN_THREADS + tid];
    tile[0][tid] = s0; tile[0][NN_THREADS + tid] = s1; tile[0][2 * NN_THREADS + tid] = s2;
    __syncthreads();

    for (int t = 0; t < n_tiles; ++t) {
        const int cur = t & 1;
        const bool more = (t + 1 < n_tiles);
        if (more) {                                               // next tile: global -> registers, hidden under compute
            const float4 *nsrc = tsrc + 3ll * TILE_GROUPS * (t + 1);
            s0 = nsrc[tid]; s1 = nsrc[NN_THREADS + tid]; s2 = nsrc[2 * NN_THREADS + tid];
        }
        const uint32_t jbase = (uint32_t)(g_begin + t * TILE_GROUPS) * 4u;
#pragma unroll 2
        for (int g = 0; g < TILE_GROUPS; ++g) {
            const float4 X = tile[cur][3 * g], Y = tile[cur][3 * g + 1], Z = tile[cur][3 * g + 2];
            const uint32_t j = jbase + 4u * (uint32_t)g;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float d0 = d2_metric(px[r], py[r], pz[r], X.x, Y.x, Z.x);
                const float d1 = d2_metric(px[r], py[r], pz[r], X.y, Y.y, Z.y);
                const float d2 = d2_metric(px[r], py[r], pz[r], X.z, Y.z, Z.z);
                const float d3 = d2_metric(px[r], py[r], pz[r], X.w, Y.w, Z.w);
                const float m = __builtin_fminf(__builtin_fminf(d0, d1), d2);
                const float nb = __builtin_fminf(__builtin_fminf(m, d3), best[r]);
                if (nb < best[r]) {                                // rare after the first tiles
                    const uint32_t k = (d0 == nb) ? 0u : (d1 == nb) ? 1u : (d2 == nb) ? 2u : 3u;
                    bidx[r] = j + k;
                    best[r] = nb;
                }
            }
        }
        if (more) {
            tile[cur ^ 1][tid] = s0; tile[cur ^ 1][NN_THREADS + tid] = s1; tile[cur ^ 1][2 * NN_THREADS + tid] = s2;
        }
        __syncthreads();
    }

#pragma unroll
    for (int r = 0; r < R; ++r) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(best[r]) << 32) | bidx[r];
        unsigned long long *dst = keys + base + r * NN_THREADS + tid;
        if (gridDim.x == 1) *dst = key;
        else atomicMin(dst, key);                                  // (d2, idx) lexicographic: lowest index on ties
    }
}

// ------------------------------------------------------------------------------------------------
// k_nn_search_filtered : same answers as k_nn_search, ~3 VALU ops per pair instead of ~6.8
// ------------------------------------------------------------------------------------------------
// Idea: a cheap score that can only be used to PROVE "this target cannot win or tie", never to pick a winner.
//   centred coordinates   qh = fl32(q - c),  ph = fl32(p - c)          (c = centre of the target bbox)
//   score                 s_j = fma(ph.x, -2qh.x, fma(ph.y, -2qh.y, fma(ph.z, -2qh.z, w_j))),  w_j = fl32(|qh_j|^2)
//                         ~ |ph - qh_j|^2 - |ph|^2                      (3 fma per pair instead of 3 sub + mul + 2 fma)
//   threshold             T = round_up( best*(1+16u) + 16u*G^2 - |ph|^2 + 1e-30 ),  G = |ph| + max_j |qh_j|,  u = 2^-24
// Claim: s_j > T  implies  d2_metric(p, q_j) > best  (strictly), so a group of 4 targets whose smallest score exceeds
// T is skipped; every other group takes the exact path (difference-form d2, lexicographic (d2, index) update).
// Proof sketch (full derivation in docs/HISTORY.md 4.1): |s_j - S_j| <= 4.01u G^2 (three fma roundings + the rounding of w_j);
// centring moves |ph-qh_j| by at most 1.01u G; the exact metric is within a factor (1 +- 5.01u) of the real squared
// distance.  8u would already suffice for both terms; 16u is used.  T is rounded towards +inf.
// Targets/queries with non-finite or astronomically large coordinates disable the filter on the host side
// (k_nn_search is used instead).
//
// Seeding: `prev` holds each point's nearest index from the previous ICP iteration; its exact distance under the
// new transform is a valid upper bound for the minimum, so the scan starts with a tight threshold and the exact
// path is taken only for real improvements and near-ties.  Any seed gives the same final answer.
constexpr double FILTER_K = 16.0 * 5.9604644775390625e-08;   // 16 u
constexpr double FILTER_ABS = 1e-30;
constexpr int FTILE_GROUPS = 256;                            // groups per LDS tile: 256 x 64 B = 16 KiB

__device__ __forceinline__ float round_up_to_float(double x)
{
    float f = (float)x;
    if ((double)f < x) {                                      // nextafter(f, +inf)
        uint32_t b = __float_as_uint(f);
        if (f > 0.f) b += 1u;
        else if (f < 0.f) b -= 1u;
        else b = 1u;
        f = __uint_as_float(b);
    }
    return f;
}

// thr3 bounds the 3-D score, thr2 the 2-D score (the kept-plane distance can only be smaller than the 3-D one, the
// rounding analysis is the same with one fma less, and G bounds the 2-D norms as well)
__device__ __forceinline__ void filter_thresholds(float best, float hu, float hv, float hd, double qmax, float &thr2,
                                                  float &thr3)
{
    if (!(best < INFINITY)) { thr2 = INFINITY; thr3 = INFINITY; return; }   // nothing known yet: nothing can be skipped
    const double P2 = (double)hu * (double)hu + (double)hv * (double)hv;
    const double P3 = P2 + (double)hd * (double)hd;
    const double G = sqrt(P3) * (1.0 + 1e-12) + qmax;
    const double base = (double)best * (1.0 + FILTER_K) + FILTER_K * G * G + FILTER_ABS;
    thr2 = round_up_to_float(base - P2);
    thr3 = round_up_to_float(base - P3);
}

// filter images of the target, per group of 4 vertices.  (u, v, d) = fax: the axis of smallest extent is dropped by
// the first-level score.   tf2: [-2qu][-2qv][qu^2+qv^2]  (tiled through LDS)     tf3: [-2qd][|q|^2]  (rare path, global)
// Padding can never pass: its W2 / W3 are 3e38.
#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
__global__ void k_pack_filter(const float *__restrict__ xyz, int nt, int n_groups_pad, float cx, float cy, float cz,
                              int au, int av, int ad, float4 *__restrict__ tf2, float4 *__restrict__ tf3,
                              double *__restrict__ block_max_q2)
{
    __shared__ double red[4];
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    double mx = 0.0;
    if (g < n_groups_pad) {
        float a[3][4], w2[4], w3[4];
        for (int k = 0; k < 4; ++k) {
            const long long v = 4ll * g + k;
            if (v < nt) {
                float q[3];
                q[0] = (float)((double)xyz[3 * v] - (double)cx);
                q[1] = (float)((double)xyz[3 * v + 1] - (double)cy);
                q[2] = (float)((double)xyz[3 * v + 2] - (double)cz);
                const double p2 = (double)q[au] * (double)q[au] + (double)q[av] * (double)q[av];
                const double q2 = p2 + (double)q[ad] * (double)q[ad];
                a[0][k] = -2.0f * q[au]; a[1][k] = -2.0f * q[av]; a[2][k] = -2.0f * q[ad];
                w2[k] = (float)p2;
                w3[k] = (float)q2;
                if (q2 > mx) mx = q2;
            } else {
                a[0][k] = 0.f; a[1][k] = 0.f; a[2][k] = 0.f; w2[k] = 3.0e38f; w3[k] = 3.0e38f;
            }
        }
        if (tf2) {                                                   // (nullptr: only the maximum is wanted -- the images are k_nn_search_filtered's, an OA_EXPERIMENTS kernel)
            tf2[3ll * g] = make_float4(a[0][0], a[0][1], a[0][2], a[0][3]);
            tf2[3ll * g + 1] = make_float4(a[1][0], a[1][1], a[1][2], a[1][3]);
            tf2[3ll * g + 2] = make_float4(w2[0], w2[1], w2[2], w2[3]);
            tf3[2ll * g] = make_float4(a[2][0], a[2][1], a[2][2], a[2][3]);
            tf3[2ll * g + 1] = make_float4(w3[0], w3[1], w3[2], w3[3]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_down(mx, off, 64); mx = o > mx ? o : mx; }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = red[0];
        for (int k = 1; k < (int)(blockDim.x >> 6); ++k) m = red[k] > m ? red[k] : m;
        block_max_q2[blockIdx.x] = m;
    }
}

// per-block bounding box of the target (min xyz, max xyz); NaN-poisoned if any coordinate is not finite
__global__ void k_bbox_partial(const float *__restrict__ xyz, int nt, float *__restrict__ out /* blocks x 6 */)
{
    __shared__ float red[4][6];
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    bool bad = false;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nt; i += gridDim.x * blockDim.x)
        for (int a = 0; a < 3; ++a) {
            const float v = xyz[3ll * i + a];
            if (!(fabsf(v) < INFINITY)) bad = true;
            lo[a] = fminf(lo[a], v); hi[a] = fmaxf(hi[a], v);
        }
    if (bad) { lo[0] = NAN; hi[0] = NAN; }
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float l = __shfl_down(lo[a], off, 64), h = __shfl_down(hi[a], off, 64);
            lo[a] = (l != l || lo[a] != lo[a]) ? NAN : fminf(lo[a], l);
            hi[a] = (h != h || hi[a] != hi[a]) ? NAN : fmaxf(hi[a], h);
        }
    }
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; ++a) { red[threadIdx.x >> 6][a] = lo[a]; red[threadIdx.x >> 6][3 + a] = hi[a]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        float v = red[0][a];
        for (int k = 1; k < (int)(blockDim.x >> 6); ++k) {
            const float o = red[k][a];
            v = (o != o || v != v) ? NAN : (a < 3 ? fminf(v, o) : fmaxf(v, o));
        }
        out[blockIdx.x * 6 + a] = v;
    }
}
#endif  // !OA_FAMILY_TU

typedef float v2f __attribute__((ext_vector_type(2)));

template <int R, int TG = FTILE_GROUPS>
__global__ __launch_bounds__(NN_THREADS, (R <= 4 ? 4 : 2)) void k_nn_search_filtered(const DevState *__restrict__ st,
                                                                   const float4 *__restrict__ src4,
                                                                   const float4 *__restrict__ tg,
                                                                   const float4 *__restrict__ tf2,
                                                                   const float4 *__restrict__ tf3,
                                                                   const float4 *__restrict__ win,
                                                                   int n_groups_pad,
                                                                   unsigned long long *__restrict__ keys)
{
    // scalar v_fma_f32 throughout: the packed form (v_pk_fma_f32) measured 3-5 % slower in this loop (docs/HISTORY.md 5)
    if (st->halt) return;
    // TG = groups of 4 targets per LDS tile: 256 for large targets, 64 for small ones (more, shorter workgroups)
    constexpr int TILE_F4 = TG * 3, LOADS = (TILE_F4 + NN_THREADS - 1) / NN_THREADS;
    // whole tiles per thread (TG = 256): the staging registers must not be predicated, or the compiler parks them in
    // scratch and the tile loop writes and re-reads 48 B per lane per tile through HBM (PMC: 4.9 GB per launch)
    constexpr bool FULL = (TILE_F4 % NN_THREADS) == 0;
    __shared__ float4 tile[2][TILE_F4];
    const int tid = threadIdx.x;
    const double qmax = st->qmax;
    const float cx = st->tc[0], cy = st->tc[1], cz = st->tc[2];
    const int au = st->fax[0], av = st->fax[1];
    const int base = blockIdx.y * (NN_THREADS * R);
    float px[R], py[R], pz[R], hu[R], hv[R], hd[R], best[R], thr2[R], thr3[R], seed_d[R];
    uint32_t bidx[R], seed_idx[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = base + r * NN_THREADS + tid;
        const float4 p = src4[i];
        co_find(st, p.x, p.y, p.z, px[r], py[r], pz[r]);    // co_find (general.py:287)
        const float h0 = (float)((double)px[r] - (double)cx);
        const float h1 = (float)((double)py[r] - (double)cy);
        const float h2 = (float)((double)pz[r] - (double)cz);
        hu[r] = au == 0 ? h0 : (au == 1 ? h1 : h2);               // kept axes of the 2-D score
        hv[r] = av == 0 ? h0 : (av == 1 ? h1 : h2);
        hd[r] = (au + av == 1) ? h2 : ((au + av == 2) ? h1 : h0); // the dropped axis is the remaining one
        best[r] = INFINITY;
        bidx[r] = IDX_NONE;
        // seed: the slot's winner record of the last search (coordinates + index, kept current by k_pair_accumulate) --
        // one coalesced 16-byte read per split where the index alone cost a scattered gather from the target array
        const float4 sw = win ? win[i] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
        if (__float_as_int(sw.w) >= 0) {
            const float d = d2_metric(px[r], py[r], pz[r], sw.x, sw.y, sw.z);
            if (d < INFINITY) { best[r] = d; bidx[r] = (uint32_t)__float_as_int(sw.w); }
        }
        seed_idx[r] = bidx[r];
        seed_d[r] = best[r];
        filter_thresholds(best[r], hu[r], hv[r], hd[r], qmax, thr2[r], thr3[r]);
    }

    int g_begin, g_end;
    split_range(n_groups_pad, TG, g_begin, g_end);
    const int n_tiles = (g_end - g_begin) / TG;
    const float4 *tsrc = tf2 + 3ll * g_begin;

    // staging registers for the next tile: named scalars (an indexed array ends up in scratch, see FULL above)
    static_assert(LOADS <= 3, "k_nn_search_filtered: tile of at most 3 float4 per thread");
    float4 stg0 = make_float4(0.f, 0.f, 0.f, 0.f), stg1 = stg0, stg2 = stg0;
#define OA_STG_EACH(OP)                                                                     \
    do {                                                                                    \
        if (LOADS > 0 && (FULL || 0 * NN_THREADS + tid < TILE_F4)) { OP(0, stg0); }         \
        if (LOADS > 1 && (FULL || 1 * NN_THREADS + tid < TILE_F4)) { OP(1, stg1); }         \
        if (LOADS > 2 && (FULL || 2 * NN_THREADS + tid < TILE_F4)) { OP(2, stg2); }         \
    } while (0)
#define OA_STG_FIRST(k, reg) reg = tsrc[(k) * NN_THREADS + tid]; tile[0][(k) * NN_THREADS + tid] = reg
    OA_STG_EACH(OA_STG_FIRST);
#undef OA_STG_FIRST
    __syncthreads();

    for (int t = 0; t < n_tiles; ++t) {
        const int cur = t & 1;
        const bool more = (t + 1 < n_tiles);
        if (more) {                                               // next tile: global -> registers, hidden under compute
            const float4 *nsrc = tsrc + 3ll * TG * (t + 1);
#define OA_STG_LOAD(k, reg) reg = nsrc[(k) * NN_THREADS + tid]
            OA_STG_EACH(OA_STG_LOAD);
#undef OA_STG_LOAD
        }
        const int gbase = g_begin + t * TG;
        // GW groups (4*GW targets) per skip test.  Level 1 (hot): 2 fma + min per pair in the kept plane; level 2 (rare):
        // the dropped axis is added for the points that passed; level 3 (rarer): the exact metric.
        constexpr int GW = 2;
        for (int g = 0; g < TG; g += GW) {
            float4 AU[GW], AV[GW], W2[GW];
#pragma unroll
            for (int k = 0; k < GW; ++k) {
                AU[k] = tile[cur][3 * (g + k)]; AV[k] = tile[cur][3 * (g + k) + 1]; W2[k] = tile[cur][3 * (g + k) + 2];
            }
            float gm[R];
            bool hit = false;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float m = INFINITY;
#pragma unroll
                for (int k = 0; k < GW; ++k) {
                    const float c0 = __builtin_fmaf(hu[r], AU[k].x, __builtin_fmaf(hv[r], AV[k].x, W2[k].x));
                    const float c1 = __builtin_fmaf(hu[r], AU[k].y, __builtin_fmaf(hv[r], AV[k].y, W2[k].y));
                    const float c2 = __builtin_fmaf(hu[r], AU[k].z, __builtin_fmaf(hv[r], AV[k].z, W2[k].z));
                    const float c3 = __builtin_fmaf(hu[r], AU[k].w, __builtin_fmaf(hv[r], AV[k].w, W2[k].w));
                    m = __builtin_fminf(m, __builtin_fminf(__builtin_fminf(c0, c1), __builtin_fminf(c2, c3)));
                }
                gm[r] = m;
                hit = hit || !(m > thr2[r]);
            }
            if (hit) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (!(gm[r] > thr2[r])) {                         // level 2: full 3-D score for these 4*GW targets
                        float m3 = INFINITY;
                        for (int k = 0; k < GW; ++k) {
                            const float4 AD = tf3[2ll * (gbase + g + k)], W3 = tf3[2ll * (gbase + g + k) + 1];
                            const float c0 = __builtin_fmaf(hu[r], AU[k].x, __builtin_fmaf(hv[r], AV[k].x, __builtin_fmaf(hd[r], AD.x, W3.x)));
                            const float c1 = __builtin_fmaf(hu[r], AU[k].y, __builtin_fmaf(hv[r], AV[k].y, __builtin_fmaf(hd[r], AD.y, W3.y)));
                            const float c2 = __builtin_fmaf(hu[r], AU[k].z, __builtin_fmaf(hv[r], AV[k].z, __builtin_fmaf(hd[r], AD.z, W3.z)));
                            const float c3 = __builtin_fmaf(hu[r], AU[k].w, __builtin_fmaf(hv[r], AV[k].w, __builtin_fmaf(hd[r], AD.w, W3.w)));
                            m3 = __builtin_fminf(m3, __builtin_fminf(__builtin_fminf(c0, c1), __builtin_fminf(c2, c3)));
                        }
                        if (!(m3 > thr3[r])) {                        // level 3: cannot be ruled out, exact metric
                            float b = best[r];
                            uint32_t bi = bidx[r];
                            for (int k = 0; k < GW; ++k) {
                                const float4 *eg = tg + 3ll * (gbase + g + k);
                                const float4 X = eg[0], Y = eg[1], Z = eg[2];
                                const uint32_t j = (uint32_t)(gbase + g + k) * 4u;
                                const float e0 = d2_metric(px[r], py[r], pz[r], X.x, Y.x, Z.x);
                                const float e1 = d2_metric(px[r], py[r], pz[r], X.y, Y.y, Z.y);
                                const float e2 = d2_metric(px[r], py[r], pz[r], X.z, Y.z, Z.z);
                                const float e3 = d2_metric(px[r], py[r], pz[r], X.w, Y.w, Z.w);
                                if (e0 < b || (e0 == b && j < bi)) { b = e0; bi = j; }
                                if (e1 < b || (e1 == b && j + 1u < bi)) { b = e1; bi = j + 1u; }
                                if (e2 < b || (e2 == b && j + 2u < bi)) { b = e2; bi = j + 2u; }
                                if (e3 < b || (e3 == b && j + 3u < bi)) { b = e3; bi = j + 3u; }
                            }
                            if (b < best[r]) filter_thresholds(b, hu[r], hv[r], hd[r], qmax, thr2[r], thr3[r]);
                            best[r] = b;
                            bidx[r] = (b < INFINITY) ? bi : IDX_NONE;     // overflowed distances (+inf) never win
                        }
                    }
                }
            }
        }
        if (more) {
#define OA_STG_STORE(k, reg) tile[cur ^ 1][(k) * NN_THREADS + tid] = reg
            OA_STG_EACH(OA_STG_STORE);
#undef OA_STG_STORE
        }
        __syncthreads();
    }
#undef OA_STG_EACH

    // A split reports when it has something to say: a better vertex than the seed, or the seed itself when it lies in
    // this split's range (exactly one split owns it, so the key is never left empty).  With 24 splits and a settled
    // pose that is one 64-bit atomic per point instead of 24 (PMC: 187 MB of HBM-side writes per launch for 8 MB of keys).
    const uint32_t own_lo = (uint32_t)g_begin * 4u, own_hi = (uint32_t)g_end * 4u;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(best[r]) << 32) | bidx[r];
        unsigned long long *dst = keys + base + r * NN_THREADS + tid;
        if (gridDim.x == 1) *dst = key;
        else {
            const bool seeded = seed_idx[r] != IDX_NONE;
            const bool improved = bidx[r] != seed_idx[r] || best[r] != seed_d[r];
            const bool owner = seeded && seed_idx[r] >= own_lo && seed_idx[r] < own_hi;
            if (!seeded || improved || owner) atomicMin(dst, key);  // (d2, idx) lexicographic: lowest index on ties
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_nn_search_sorted : k_nn_search_filtered with one more, cheaper level in front, over a target in sorted order
// ------------------------------------------------------------------------------------------------
// Every (source, target) pair still gets its own arithmetic; what differs is the ORDER of the target and the first test.  (How the
// kernel came to this form, round by round and with each step's numbers: docs/HISTORY.md and DESIGN.md section 3.1.)
// The target's images lie in the order of the coordinate u along the cloud's longest axis (a 30-bit quantised key, stable sort; the
// order only matters for speed -- any permutation gives the same answers), so an LDS tile of 1024 vertices is a thin slab in u; the
// source points a wave owns are neighbours in space (Morton order).  Within every block of 256 positions, positions 1 .. n-1 are in
// the order of the second coordinate v (k_sort_blocks_v, OA_NN_VCHUNK=1).
//   level 0 (hot loop)  the 1-D gap along u of a point -- or a pair of the lane's points -- and a vertex or an image of several,
//                       folded over a block of 256 vertices into one minimum and ONE compare (oa_level0.hpp).  With base the
//                       right-hand side of filter_thresholds (best inflated by every rounding allowance of the 2-D / 3-D scores),
//                       a vertex is a proven loser when its REAL gap t = |qu - hu| has t^2 > base (the distance along one axis
//                       never exceeds the 3-D distance).  Every kind computes in float32 a value that exceeds the smallest real
//                       gap it stands for by no more than a stated allowance, and thr1 (sorted_thresholds) carries that
//                       allowance: value > threshold proves every vertex behind it a loser.  (Flushed denormals only make a gap
//                       smaller: fewer pairs skipped, never a wrong one.)  For all slabs but the few around the wave's own u
//                       range every block fails here.  The four kinds (sorted_level0 below says which instance runs which):
//     per vertex          a = |fl(qu - hu)| against thr1, from the tfs tile itself: fl(qu - hu) = (qu - hu)(1 + e), |e| <= 2^-24,
//                         and thr1 >= round_up(sqrt(base)(1 + 2^-22)).  One subtract and half a v_min3_f32 per pair.
//     vertex pairs        positions (4g, 4g+1) and (4g+2, 4g+3) as midpoint and half-width {m, w} of their u (tmw, k_pack_sorted):
//                         min(|q1 - hu|, |q2 - hu|) = ||m - hu| - w| in closed form; in float32 within A = 2^-24 (3 qmax + |hu|) of
//                         it, and thr1 = round_up((sqrt(base) + A)(1 + 2^-22)).  A pair with padding has w = 0: a single gap.
//                         1.25 instructions per pair.  Proof: oa_pairgap.hpp.
//     ... x point pairs   the same identity once more on the lane's points 2p, 2p + 1 ({hm, hw} and an allowance per pair,
//                         k_sorted_point_setup): the signed t = ||m - hm| - hw| - w never exceeds the smallest of the four gaps
//                         by more than the allowance, so t > quad_threshold(the two thr1, allowance) rules out both vertices for
//                         both points.  0.88 instructions per pair.  Proof: oa_quadgap.hpp.
//     images x point pairs  one image {mm, ww, ws} per SORTED_IMAGE_V = 16 sorted positions (toct, k_group_images): 0 <= ww <= c
//                         and every vertex of the group within ws of mm + ww or mm - ww, as stored; the set-up keeps hw' =
//                         max(hw, c) and adds e = hw' - hw to the pair's allowance.  The signed t = |||mm - hm| - hw'| - ww| - ws
//                         never exceeds the smallest of the 32 gaps by more than e and the allowance.  Four subtracts per 32
//                         pairs, a v_min3_f32 per 64: 0.14 instructions per pair.  An image never spans more than level 0v's
//                         chunk.  Proof: oa_octgap.hpp, (1')-(6').
//                       The point-pair kinds mark a hit block for BOTH points of a pair; levels 0v-3 decide per point with their own
//                       thr1.  In every kind each vertex's and each point's own coordinate is in an arithmetic test, every tile is
//                       visited, nothing is decided from a block's or a tile's bounds.
//   level 0v (rare)     for a block some lane hit (VCHUNK): the same gap along v, a_j = fl32(hv - qv_j) against the same thr1, from
//                       the ENDS of each chunk of 4 SORTED_VCG vertices.  Positions 1 .. n-1 of a block are in the order of qv, and
//                       rounding is monotone, so a_j does not increase along a chunk: with F, L its first and last, every
//                       |a_j| >= L when L > 0 and >= -F when F < 0.  max(L, -F) > thr1 (true; NaN: false) therefore proves
//                       min |a_j| > thr1 -- what level 0's proof needs -- and the chunk is ruled out; a chunk with F >= 0 >= L
//                       passes (one whose interior straddles hv with no vertex near it passes in vain).  Position 0 of a block is
//                       not in that order and is tested on its own; a block with padding is not tested (its chunks that hold a
//                       vertex pass); thr1 = +inf (unseeded) passes every chunk.  (A NaN v sorts to a block's ends; such a vertex
//                       never wins, and max() of a NaN and a number is the number, which bounds the rest alone.)
//   levels 1, 2, 3      as k_nn_search_filtered (2-D score, 3-D score, exact metric), reached by ~6 % of the blocks at 1M <-> 1M.
//                       VCHUNK: level 1 per chunk of level 0v, then levels 2-3 group by group; else group by group for the whole
//                       block.
// Indices: position j of the sorted images holds original vertex tidx[j]; the exact path compares and reports ORIGINAL indices
// (lowest index on ties, as everywhere).  A split owns a seed when seed index mod splits = split (no position lookup).
// Tiles are visited middle-out from the slab nearest to the workgroup's first point: an unseeded search (the first iteration of a
// loop) then finds a tight best at once instead of sweeping towards it, and a seeded one tightens its seeds at once (the order
// never changes an answer, only how soon the thresholds are final).

// The kinds of level 0, and THE decision which instance folds which -- asked by the kernel (its fold, its tile of images), by
// k_sorted_point_setup (whether a point pair's record is capped) and by the launcher (which array of images to pass); the upload
// builds every kind's images, since a target does not know its sources' R.  R = 8 exists in the experiments library only.
enum class Level0 { PerVertex, VertexPairs, PointPairs, Images };
constexpr Level0 sorted_level0(int R, bool VCHUNK)
{
    return !VCHUNK ? Level0::PerVertex : R == 1 ? Level0::VertexPairs : R <= 4 ? Level0::Images : Level0::PointPairs;
}
constexpr bool level0_on_point_pairs(Level0 k) { return k == Level0::PointPairs || k == Level0::Images; }
constexpr int SORTED_IMAGE_V = 16;        // sorted positions per image (4 / 8 / 16: 11.52 / 7.87 / 6.20 ms per step, profiles/r19a_vertex_octets.txt)
constexpr int SORTED_GW = 64;             // groups of 4 sorted vertices per block, level 0's skip test (the sweep: at the kernel)
constexpr int SORTED_VCG = 4;             // groups per chunk of level 0v (2 / 4 / 8: 25.46 / 24.99 / 24.94 ms at 1M <-> 1M, profiles/r08a_vends.txt)
constexpr double SORTED_OCT_CAP = 1.0;    // the images' cap c in mean half-spans of a block (any value >= 0 gives the same answers; sweep: profiles/r18a_vertex_quads.txt)
// float4 of level 0's own images per tile of TG groups (none: the per-vertex kind reads the tfs tile)
constexpr int level0_tile_f4(Level0 k, int TG) { return k == Level0::PerVertex ? 0 : k == Level0::Images ? TG * 3 / SORTED_IMAGE_V : TG; }
static_assert(4 * SORTED_VCG % SORTED_IMAGE_V == 0, "an image never spans more than level 0v's chunk");
#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
__global__ void k_sort_keys_axis(const float *__restrict__ xyz, int nt, int axis, double lo, double scale, unsigned *__restrict__ keys)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nt) return;
    double t = ((double)xyz[3ll * i + axis] - lo) * scale;
    t = t < 0.0 ? 0.0 : (t > 1073741823.0 ? 1073741823.0 : t);
    keys[i] = (unsigned)t;
}

// images in sorted order, per group of 4 positions: tfs [qu][-2qv][qu^2+qv^2] (LDS tiles; -2qu is exact from qu), tf3s [-2qd][|q|^2],
// tgs [x][y][z] (exact), tidx original indices.  Same centring and roundings as k_pack_filter / k_pack_target.
// tmw: level 0's pair images {m01, w01, m23, w23} of the group's positions (0, 1) and (2, 3), from the same qu
// (pair_image, oa_pairgap.hpp) -- positions of the FINAL order, k_sort_blocks_v's included.  (toct: k_group_images, below.)
__global__ void k_pack_sorted(const float *__restrict__ xyz, int nt, int n_groups_pad, const int *__restrict__ order, float cx, float cy,
                              float cz, int au, int av, int ad, float4 *__restrict__ tfs, float4 *__restrict__ tf3s,
                              float4 *__restrict__ tgs, int4 *__restrict__ tidx, float4 *__restrict__ tmw)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups_pad) return;
    float a[3][4], qu[4], w2[4], w3[4], e[3][4];
    int id[4];
    for (int k = 0; k < 4; ++k) {
        const long long j = 4ll * g + k;
        if (j < nt) {
            const int v = order[j];
            id[k] = v;
            float q[3];
            e[0][k] = xyz[3ll * v]; e[1][k] = xyz[3ll * v + 1]; e[2][k] = xyz[3ll * v + 2];
            q[0] = (float)((double)e[0][k] - (double)cx);
            q[1] = (float)((double)e[1][k] - (double)cy);
            q[2] = (float)((double)e[2][k] - (double)cz);
            const double p1 = (double)q[au] * (double)q[au];
            const double p2 = p1 + (double)q[av] * (double)q[av];
            const double q2 = p2 + (double)q[ad] * (double)q[ad];
            a[0][k] = -2.0f * q[au]; a[1][k] = -2.0f * q[av]; a[2][k] = -2.0f * q[ad];
            qu[k] = q[au]; w2[k] = (float)p2; w3[k] = (float)q2;
        } else {                                                  // padding can never pass a level, nor win
            id[k] = -1;
            e[0][k] = e[1][k] = e[2][k] = INFINITY;
            a[0][k] = a[1][k] = a[2][k] = 0.f;
            qu[k] = PAIR_PAD_U;                                   // (1e18: far, and -2 qu stays finite; the tail of the order -- keys clamp)
            w2[k] = w3[k] = 3.0e38f;
        }
    }
    tfs[3ll * g] = make_float4(qu[0], qu[1], qu[2], qu[3]);
    tfs[3ll * g + 1] = make_float4(a[1][0], a[1][1], a[1][2], a[1][3]);
    tfs[3ll * g + 2] = make_float4(w2[0], w2[1], w2[2], w2[3]);
    tf3s[2ll * g] = make_float4(a[2][0], a[2][1], a[2][2], a[2][3]);
    tf3s[2ll * g + 1] = make_float4(w3[0], w3[1], w3[2], w3[3]);
    tgs[3ll * g] = make_float4(e[0][0], e[0][1], e[0][2], e[0][3]);
    tgs[3ll * g + 1] = make_float4(e[1][0], e[1][1], e[1][2], e[1][3]);
    tgs[3ll * g + 2] = make_float4(e[2][0], e[2][1], e[2][2], e[2][3]);
    tidx[g] = make_int4(id[0], id[1], id[2], id[3]);
    float4 mw;
    pair_image(qu[0], id[0] >= 0, qu[1], id[1] >= 0, mw.x, mw.y);
    pair_image(qu[2], id[2] >= 0, qu[3], id[3] >= 0, mw.z, mw.w);
    tmw[g] = mw;
}

// toct: level 0's image {mm, ww, ws} of every V = SORTED_IMAGE_V consecutive positions of the FINAL order under the cap oct_c
// (group_image, oa_octgap.hpp), from the qu k_pack_sorted left in tfs and the indices in tidx (a position is real when its index
// is >= 0); three float4 per four images -- their four mm, their four ww, their four ws.  One thread per image, n_images =
// 4 n_groups_pad / V (a multiple of 4: n_groups_pad is a multiple of 256).
__global__ void k_group_images(const float4 *__restrict__ tfs, const int4 *__restrict__ tidx, int n_images, float oct_c, float4 *__restrict__ toct)
{
    constexpr int V = SORTED_IMAGE_V;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_images) return;
    float q[V];
    int n_real = 0;
#pragma unroll
    for (int k = 0; k < V / 4; ++k) {
        const long long g = (long long)i * (V / 4) + k;
        const float4 Q = tfs[3ll * g];
        const int4 J = tidx[g];
        q[4 * k] = Q.x; q[4 * k + 1] = Q.y; q[4 * k + 2] = Q.z; q[4 * k + 3] = Q.w;
        n_real += (J.x >= 0) + (J.y >= 0) + (J.z >= 0) + (J.w >= 0);     // (padding only ever follows the vertices)
    }
    float mm, ww, ws;
    group_image<V>(q, n_real, oct_c, mm, ww, ws);
    float *oc = reinterpret_cast<float *>(toct + 3ll * (i >> 2)) + (i & 3);
    oc[0] = mm; oc[4] = ww; oc[8] = ws;
}
#endif  // !OA_FAMILY_TU

// thr1: the 1-D gap's threshold (header above; with level 0's allowance for a pair's gap, which the single gaps of level 0v and of
// the VCHUNK = false instances do not need -- a threshold that is too high only prunes less); thr2: the 2-D score's
// (filter_thresholds).  The 3-D score's is derived from thr2 where it is needed.
__device__ __forceinline__ void sorted_thresholds(float best, float hu, float hv, float hd, double qmax, float &thr1, float &thr2)
{
    if (!(best < INFINITY)) { thr1 = INFINITY; thr2 = INFINITY; return; }
    const double P2 = (double)hu * (double)hu + (double)hv * (double)hv;
    const double P3 = P2 + (double)hd * (double)hd;
    const double G = sqrt(P3) * (1.0 + 1e-12) + qmax;
    const double base = (double)best * (1.0 + FILTER_K) + FILTER_K * G * G + FILTER_ABS;
    thr1 = round_up_to_float((sqrt(base) + pair_allowance(qmax, hu)) * (1.0 + 0x1p-22));
    thr2 = round_up_to_float(base - P2);
}

// Level 1 of the sorted kernels for ONE point and ONE group of 4 sorted positions (AU / AV / W2: the group's -2qu, -2qv,
// qu^2+qv^2): the smallest of the four 2-D scores.  The group is ruled out when it is > thr2 (a NaN is not: it goes on).
__device__ __forceinline__ float sorted_level1_min(const float4 AU, const float4 AV, const float4 W2, float hu, float hv)
{
    const float c0 = __builtin_fmaf(hu, AU.x, __builtin_fmaf(hv, AV.x, W2.x));
    const float c1 = __builtin_fmaf(hu, AU.y, __builtin_fmaf(hv, AV.y, W2.y));
    const float c2 = __builtin_fmaf(hu, AU.z, __builtin_fmaf(hv, AV.z, W2.z));
    const float c3 = __builtin_fmaf(hu, AU.w, __builtin_fmaf(hv, AV.w, W2.w));
    return __builtin_fminf(__builtin_fminf(c0, c1), __builtin_fminf(c2, c3));
}

// Levels 2 and 3 for a group level 1 could not rule out.  Returns true when the point's best improved (its thresholds are then
// already renewed).
__device__ __forceinline__ bool sorted_finish_level2(const float4 AU, const float4 AV, long long group,
                                                     const float4 *__restrict__ tf3s, const float4 *__restrict__ tgs,
                                                     const int4 *__restrict__ tidx, const float4 *__restrict__ pco, float hu, float hv,
                                                     float hd, double qmax, float &best, uint32_t &bidx, float &thr1, float &thr2)
{
    // level 2: the 3-D score
    const float4 AD = tf3s[2ll * group], W3 = tf3s[2ll * group + 1];
    const float e0s = __builtin_fmaf(hu, AU.x, __builtin_fmaf(hv, AV.x, __builtin_fmaf(hd, AD.x, W3.x)));
    const float e1s = __builtin_fmaf(hu, AU.y, __builtin_fmaf(hv, AV.y, __builtin_fmaf(hd, AD.y, W3.y)));
    const float e2s = __builtin_fmaf(hu, AU.z, __builtin_fmaf(hv, AV.z, __builtin_fmaf(hd, AD.z, W3.z)));
    const float e3s = __builtin_fmaf(hu, AU.w, __builtin_fmaf(hv, AV.w, __builtin_fmaf(hd, AD.w, W3.w)));
    // (the 3-D threshold from the 2-D one: base - P3 <= thr2 - hd^2, rounded up -- a register per point less than keeping it; a
    //  threshold that is too high only prunes less)
    if (__builtin_fminf(__builtin_fminf(e0s, e1s), __builtin_fminf(e2s, e3s)) > round_up_to_float((double)thr2 - (double)hd * (double)hd))
        return false;
    // level 3: cannot be ruled out, exact metric, original indices
    float b = best;
    uint32_t bi = bidx;
    const float4 *eg = tgs + 3ll * group;
    const float4 X = eg[0], Y = eg[1], Z = eg[2];
    const int4 J = tidx[group];
    const float4 P = *pco;                                         // co_find of the point, from its record: only here is it needed
    const float px = P.x, py = P.y, pz = P.z;
    const float e0 = d2_metric(px, py, pz, X.x, Y.x, Z.x);
    const float e1 = d2_metric(px, py, pz, X.y, Y.y, Z.y);
    const float e2 = d2_metric(px, py, pz, X.z, Y.z, Z.z);
    const float e3 = d2_metric(px, py, pz, X.w, Y.w, Z.w);
    if (e0 < b || (e0 == b && (uint32_t)J.x < bi)) { b = e0; bi = (uint32_t)J.x; }
    if (e1 < b || (e1 == b && (uint32_t)J.y < bi)) { b = e1; bi = (uint32_t)J.y; }
    if (e2 < b || (e2 == b && (uint32_t)J.z < bi)) { b = e2; bi = (uint32_t)J.z; }
    if (e3 < b || (e3 == b && (uint32_t)J.w < bi)) { b = e3; bi = (uint32_t)J.w; }
    const bool improved = b < best;
    if (improved) sorted_thresholds(b, hu, hv, hd, qmax, thr1, thr2);
    best = b;
    bidx = (b < INFINITY) ? bi : IDX_NONE;                        // overflowed distances (+inf) never win
    return improved;
}

// Levels 1 .. 3 for ONE point and ONE group, one after the other.
__device__ __forceinline__ bool sorted_finish_group(const float4 AU, const float4 AV, const float4 W2, long long group,
                                                    const float4 *__restrict__ tf3s, const float4 *__restrict__ tgs,
                                                    const int4 *__restrict__ tidx, const float4 *__restrict__ pco, float hu, float hv,
                                                    float hd, double qmax, float &best, uint32_t &bidx, float &thr1, float &thr2)
{
    if (sorted_level1_min(AU, AV, W2, hu, hv) > thr2) return false;
    return sorted_finish_level2(AU, AV, group, tf3s, tgs, tidx, pco, hu, hv, hd, qmax, best, bidx, thr1, thr2);
}

// Everything k_nn_search_sorted needs to know about a point that does not depend on the split, once per search instead of once
// per (split, block) item -- 136 times per point in a seeded 1M <-> 1M launch: co_find, the centred coordinates, the seed and
// its distance, the thresholds.  One RECORD per slot, three float4 in three arrays of ns_pad entries (rec, rec + ns_pad,
// rec + 2 ns_pad):
//   [0] hu, hv, hd, the slot's index (int bits)     [1] best, bidx (uint bits), thr1, thr2     [2] px, py, pz (co_find), 0
// and, where level 0 folds point pairs (sorted_level0), a fourth array, rec + 3 ns_pad: per lane and pair of its points (2p, 2p + 1),
// at first + 64 p + lane of the wave's records, {hm, hw, allowance, 0} -- the pair's image along u and what rounding can add to its
// gap (oa_quadgap.hpp); for the image kind {hm, max(hw, c), allowance + e, 0} with the cap c = oct_c the target's images were built
// with (oa_octgap.hpp) -- a launch argument, read from the target beside its images: the bound needs the SAME c on both sides, and
// the images may be built while a sequence is open (oa_set_search_mode), after the device state was staged.
// The seed is the slot's winner record (pass 0) or what k_nn_seed_sorted left in keys (pass 2: this kernel runs after it).
// The arithmetic is the item prologue's of before, through the same device functions: the same floats.
// WHERE a slot's record lies decides which lane takes it as its point r: record first + 64 r + lane of a wave's 64 R records
// is point r of that lane.  ranked: the wave's slots in the order of their u (the coordinate the target is sorted along) AT THE
// CURRENT POSE, so that point r of all lanes is the r-th slice of the wave's extent in u -- a quarter (R = 4) of the slabs a
// plain run of 64 consecutive slots reaches into (level 1 runs per point r and wave).  rank = number of slots with a smaller
// (key, position): a permutation whatever the values (NaN included).  Not ranked (OA_NN_WAVE_ORDER=0): record i is slot i.
// One wave per 64 R slots.
// (The order over a whole workgroup's 256 R slots -- sixteen thinner slices -- measured slower in round 5, 32.0 against 31.1 ms
// per iteration at 1M <-> 1M: the lanes of a point r then spread over the workgroup's whole extent in the other two axes and
// levels 2 / 3 run for more (wave, group) combinations.)
template <int R>
__global__ __launch_bounds__(64) void k_sorted_point_setup(const DevState *__restrict__ st, const float4 *__restrict__ src4,
                                                           const float4 *__restrict__ win, const unsigned long long *__restrict__ keys,
                                                           int au, int av, int pass, int ranked, int ns_pad, int ns, float4 *__restrict__ rec,
                                                           float oct_c)
{
    if (st->halt) return;
    constexpr int N = 64 * R;
    __shared__ uint32_t key[N];
    constexpr Level0 L0 = sorted_level0(R, true);                  // (the pairs' records are read by the VCHUNK instances alone)
    __shared__ float pu[level0_on_point_pairs(L0) ? N : 1];        // the records' hu in the order the lanes read them
    const int t = threadIdx.x;
    const int first = (int)blockIdx.x * N;
    const double qmax = st->qmax;
    const float cx = st->tc[0], cy = st->tc[1], cz = st->tc[2];
    float4 ra[R], rb[R], rc[R];
    uint32_t mine[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = first + r * 64 + t;
        const float4 p = src4[i];
        float px, py, pz;
        co_find(st, p.x, p.y, p.z, px, py, pz);                    // co_find (general.py:287)
        const float h0 = (float)((double)px - (double)cx);
        const float h1 = (float)((double)py - (double)cy);
        const float h2 = (float)((double)pz - (double)cz);
        const float hu = au == 0 ? h0 : (au == 1 ? h1 : h2);
        const float hv = av == 0 ? h0 : (av == 1 ? h1 : h2);
        const float hd = (au + av == 1) ? h2 : ((au + av == 2) ? h1 : h0);
        float best = INFINITY;
        uint32_t bidx = IDX_NONE;
        const float4 sw = (win && pass == 0) ? win[i] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
        if (__float_as_int(sw.w) >= 0) {
            const float d = d2_metric(px, py, pz, sw.x, sw.y, sw.z);
            if (d < INFINITY) { best = d; bidx = (uint32_t)__float_as_int(sw.w); }
        }
        if (pass == 2) {
            const unsigned long long k = keys[i];
            const float kd = __uint_as_float((uint32_t)(k >> 32));
            if ((uint32_t)k != IDX_NONE && kd < INFINITY) { best = kd; bidx = (uint32_t)k; }
        }
        float thr1, thr2;
        sorted_thresholds(best, hu, hv, hd, qmax, thr1, thr2);
        ra[r] = make_float4(hu, hv, hd, __int_as_float(i));
        rb[r] = make_float4(best, __uint_as_float(bidx), thr1, thr2);
        rc[r] = make_float4(px, py, pz, 0.f);
        const uint32_t b = __float_as_uint(hu);
        mine[r] = (b & 0x80000000u) ? ~b : (b | 0x80000000u);     // unsigned order = float order (NaNs at the ends: still a total order)
    }
    int rank[R];
#pragma unroll
    for (int r = 0; r < R; ++r) rank[r] = ranked ? 0 : r * 64 + t;
    if (ranked) {                                                  // (uniform)
#pragma unroll
        for (int r = 0; r < R; ++r) key[r * 64 + t] = mine[r];
        __syncthreads();
        for (int j = 0; j < N; ++j) {
            const uint32_t k = key[j];                             // (broadcast read)
#pragma unroll
            for (int r = 0; r < R; ++r) rank[r] += (k < mine[r] || (k == mine[r] && j < r * 64 + t)) ? 1 : 0;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {                                  // (rank < 64 R: inside the wave's own records)
        rec[first + rank[r]] = ra[r];
        rec[ns_pad + first + rank[r]] = rb[r];
        rec[2 * ns_pad + first + rank[r]] = rc[r];
    }
    if constexpr (level0_on_point_pairs(L0)) {
        // the lane's point pairs (2p, 2p + 1) -- {hm, hw, allowance, 0} in record first + 64 p + lane of a fourth array
        // -- formed from the records the search's lane will hold, first + 64 r + lane, so after the ranking.  A pair without a
        // claim (oa_quadgap.hpp, (6): a hu that is not finite; a padding slot of the source beside a real one) gets the
        // allowance +inf: its threshold is +inf whatever its points' thr1 become
        __syncthreads();                                           // (the ranking's reads of key are done)
#pragma unroll
        for (int r = 0; r < R; ++r) pu[rank[r]] = ra[r].x;
#pragma unroll
        for (int r = 0; r < R; ++r) key[rank[r]] = (first + r * 64 + t < ns) ? 1u : 0u;
        __syncthreads();
#pragma unroll
        for (int p = 0; p < R / 2; ++p) {
            const float h1 = pu[128 * p + t], h2 = pu[128 * p + 64 + t];
            const bool claim = (h1 - h1 == 0.0f) && (h2 - h2 == 0.0f) && key[128 * p + t] == key[128 * p + 64 + t];
            float hm, hw;
            if constexpr (L0 == Level0::Images) {
                // {hm, hw' = max(hw, c), allowance + e, 0} -- the half-width under the target's cap and what the cap adds
                // to the pair's reach, in the allowance's place (oa_octgap.hpp (2), (3)): quad_threshold is fed as before
                double e;
                const float c = oct_c;
                point_pair_image_capped(h1, h2, c, hm, hw, e);
                rec[3 * ns_pad + first + 64 * p + t] = make_float4(hm, hw, claim ? round_up_to_float(oct_allowance(qmax, h1, h2, c) + e) : INFINITY, 0.f);
            } else {
                point_pair_image(h1, h2, hm, hw);
                rec[3 * ns_pad + first + 64 * p + t] = make_float4(hm, hw, claim ? round_up_to_float(quad_allowance(qmax, h1, h2)) : INFINITY, 0.f);
            }
        }
    }
}

// Seeds for the first search of a loop: every point against the ONE tile of the sorted images whose slab holds its own u (exact
// metric, original indices, lowest index on ties) -> keys.  1024 pairs per point instead of N_t; what it leaves is a distance really
// achieved (a valid starting best for k_nn_search_sorted pass 2), typically a few times the true nearest distance.
template <int TG>
__global__ __launch_bounds__(256) void k_nn_seed_sorted(const DevState *__restrict__ st, const float4 *__restrict__ src4, int ns_pad,
                                                        const float4 *__restrict__ tgs, const float4 *__restrict__ tfs,
                                                        const int4 *__restrict__ tidx, int n_groups_pad, int au,
                                                        unsigned long long *__restrict__ keys)
{
    if (st->halt) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns_pad) return;
    const float4 p = src4[i];
    float px, py, pz;
    co_find(st, p.x, p.y, p.z, px, py, pz);
    const float h[3] = { (float)((double)px - (double)st->tc[0]), (float)((double)py - (double)st->tc[1]), (float)((double)pz - (double)st->tc[2]) };
    const float hu = au == 0 ? h[0] : (au == 1 ? h[1] : h[2]);
    const int tiles = n_groups_pad / TG;
    int a = 0, b = tiles;                                          // first tile that starts beyond hu
    while (a < b) { const int mid = (a + b) >> 1; if (tfs[3ll * TG * mid].x <= hu) a = mid + 1; else b = mid; }
    const long long g0 = (long long)(a > 0 ? a - 1 : 0) * TG;
    float best = INFINITY;
    uint32_t bi = IDX_NONE;
    for (int g = 0; g < TG; ++g) {
        const float4 *eg = tgs + 3ll * (g0 + g);
        const float4 X = eg[0], Y = eg[1], Z = eg[2];
        const int4 J = tidx[g0 + g];
        const float e0 = d2_metric(px, py, pz, X.x, Y.x, Z.x), e1 = d2_metric(px, py, pz, X.y, Y.y, Z.y);
        const float e2 = d2_metric(px, py, pz, X.z, Y.z, Z.z), e3 = d2_metric(px, py, pz, X.w, Y.w, Z.w);
        if (e0 < best || (e0 == best && (uint32_t)J.x < bi)) { best = e0; bi = (uint32_t)J.x; }
        if (e1 < best || (e1 == best && (uint32_t)J.y < bi)) { best = e1; bi = (uint32_t)J.y; }
        if (e2 < best || (e2 == best && (uint32_t)J.z < bi)) { best = e2; bi = (uint32_t)J.z; }
        if (e3 < best || (e3 == best && (uint32_t)J.w < bi)) { best = e3; bi = (uint32_t)J.w; }
    }
    if (best < INFINITY && bi != IDX_NONE) {                       // (pads: +inf coordinates, index -1 -- never a seed)
        const unsigned long long key = ((unsigned long long)__float_as_uint(best) << 32) | bi;
        if (key < keys[i]) keys[i] = key;                          // (keys: KEY_EMPTY, or what an earlier pass left)
    }
}

// The work queue of k_nn_search_sorted (round 6).  One workgroup per (split, block of 1024 source points) in launch order left the chip
// 14 % (125k-point shard) to 9 % (1M points) short of the sum of its workgroups' own times (per-workgroup stamps, profiles/r06h):
// a workgroup whose points have their own slabs in its split runs levels 1-3 and lives 3.5x as long as one that only proves
// everything away at level 0 (a third of all slot time is theirs); with the hardware handing workgroups to the XCDs in strict
// rotation, slots stand empty behind a full XCD (6-8 % of them at any time), and the launch ends on a few long workgroups (the last
// twentieth of its span runs a third full).  So: as many workgroups as the chip holds, each taking (split, block) items off a
// queue until none is left -- block after block, a block's items in the order of the distance of the split from the block's own slab
// (its long items first).  NOT the long items of all blocks first: a long item waits on memory, a short one saturates the vector
// ALU, and a CU that holds both kinds does better than two CUs with one kind each (all long items first: 4.27 instead of 3.99 ms for
// the 125k-point shard, short items 58 us beside long ones and 75 us among themselves).  Eight queues, one per residue of the split
// index mod 8, and a workgroup serves the queue of its own XCD first (XCC_ID): a split's tiles stay in one L2, as they did when the
// launch order itself was the mapping.  The answers cannot depend on who does what: keys[] is merged with atomicMin.
// Measured (profiles/r06h): 1M <-> 1M 27.6 -> 26.6 ms per search, config 5's shard 58.7 -> 57.3, the 125k shard 3.98 -> 3.93.
// k_sorted_block_homes: per block of NN_THREADS x R slots the split that holds the u of its slot 0 at the current pose
// (homes[2 y]) and the tile that does (homes[2 y + 1]: where an item starts its middle-out visit), and the queues' counters back
// to zero (it runs in front of every launch).
constexpr int SORTED_QUEUES = 8, SORTED_QUEUE_STRIDE = 16;       // (counters 64 bytes apart)
#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
__global__ void k_sorted_block_homes(const DevState *__restrict__ st, const float4 *__restrict__ src4, int n_blocks, int block_slots,
                                     const float4 *__restrict__ tfs, int n_groups_pad, int tg, int au, int n_splits,
                                     int *__restrict__ homes, int *__restrict__ qcnt)
{
    const int y = blockIdx.x * blockDim.x + threadIdx.x;
    if (y < SORTED_QUEUES) qcnt[y * SORTED_QUEUE_STRIDE] = 0;
    if (y >= n_blocks) return;
    const float4 p = src4[(long long)y * block_slots];
    float px, py, pz;
    co_find(st, p.x, p.y, p.z, px, py, pz);
    const float hu = au == 0 ? (float)((double)px - (double)st->tc[0]) : (au == 1 ? (float)((double)py - (double)st->tc[1]) : (float)((double)pz - (double)st->tc[2]));
    const int tiles = n_groups_pad / tg;
    int a = 0, b = tiles;                                          // first tile that starts beyond hu (NaN: tile 0 -- any home is a valid order)
    while (a < b) { const int mid = (a + b) >> 1; if (tfs[3ll * tg * mid].x <= hu) a = mid + 1; else b = mid; }
    const long long tile = a > 0 ? a - 1 : 0;
    int sp = (int)(tile * n_splits / tiles);                       // the split whose range [s tiles / S, (s + 1) tiles / S) holds the tile
    while (sp + 1 < n_splits && (long long)(sp + 1) * tiles / n_splits <= tile) ++sp;
    while (sp > 0 && (long long)sp * tiles / n_splits > tile) --sp;
    homes[2 * y] = sp;
    homes[2 * y + 1] = (int)tile;
}
#endif  // !OA_FAMILY_TU

// Blocks of the sorted images in the order of v (round 7, OA_NN_VCHUNK=1): the positions of every SORTED_VBLOCK consecutive
// vertices -- the block level 0 tests in the smallest tile (64 groups) -- ordered by the centred float32 coordinate along the
// second axis v (ties: the u position), so that level 0v (k_nn_search_sorted) finds a point's few vertices near it in v in a few
// chunks of 16.  A block holds the same set of vertices as before, so level 0's decisions are unchanged (a minimum does not depend
// on the order), and position 0 of every block stays where it is: a tile's first vertex is the one the binary searches for a
// point's home tile read (tfs[3 TG t].x: k_sorted_block_homes, k_nn_seed_sorted).  Padding
// (positions >= nt) is only ever at the tail of the last block and stays there.  One workgroup per block, a rank sort in LDS;
// at upload only.
constexpr int SORTED_VBLOCK = 4 * (SORTED_GW < 64 ? SORTED_GW : 64);
#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
__global__ __launch_bounds__(SORTED_VBLOCK) void k_sort_blocks_v(const float *__restrict__ xyz, int nt, int av, float cv,
                                                                 int *__restrict__ order)
{
    __shared__ uint32_t key[SORTED_VBLOCK];
    const int t = threadIdx.x;
    const long long first = (long long)blockIdx.x * SORTED_VBLOCK;
    const int n = (int)(nt - first < SORTED_VBLOCK ? nt - first : SORTED_VBLOCK);   // positions of this block that hold vertices
    int id = -1;
    uint32_t mine = 0xffffffffu;
    if (t < n) {
        id = order[first + t];
        const uint32_t b = __float_as_uint((float)((double)xyz[3ll * id + av] - (double)cv));   // (k_pack_sorted's rounding)
        mine = (b & 0x80000000u) ? ~b : (b | 0x80000000u);         // unsigned order = float order
    }
    key[t] = mine;
    __syncthreads();                                               // (every read of order is done: the writes below may land in place)
    if (t < 1 || t >= n) return;
    int rank = 1;
    for (int k = 1; k < n; ++k) {
        const uint32_t o = key[k];                                 // (broadcast read)
        rank += (o < mine || (o == mine && k < t)) ? 1 : 0;
    }
    order[first + rank] = id;
}
#endif  // !OA_FAMILY_TU

// ---- the stages of k_nn_search_sorted that stand on their own, in the order the kernel calls them; level 0's folds: oa_level0.hpp.
// (The compiler optimises a function before it inlines it, so a stage moved out of the kernel is not compiled as it was inside:
//  loading the points, the per-vertex fold and levels 1-3 for a chunk stay written out in the body, each with what moving it cost;
//  profiles/r20a_sorted_stages.txt.) ---------------------------------------------------------------------------------------------

// Taking an item off the work queue (above): false when every queue is dry, else the item in {split, yblk}.  For the whole
// workgroup (it holds a barrier); thread 0 pops, s_item carries the item and, in [2], the queues found dry so far.
__device__ __forceinline__ bool sorted_take_item(int tid, int *qcnt, const int *__restrict__ homes, int n_splits, int n_blocks, int *s_item,
                                                 int &split, int &yblk)
{
    if (tid == 0) {
        // SORTED_QUEUES queues when they divide the splits (else one): queue q holds the splits s = q + nq j; item p of a queue
        // is block p / per_q at rank p mod per_q, rank k being the split k steps (0, +1, -1, +2, ...) from the block's own
        const int nq = (n_splits % SORTED_QUEUES == 0) ? SORTED_QUEUES : 1, per_q = n_splits / nq;
        const int q_len = per_q * n_blocks;
        unsigned xcc = 0;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        int got = -1, got_y = 0;
        unsigned q_dry = (unsigned)s_item[2];
        for (int a = 0; a < nq && got < 0; ++a) {
            const int q = (int)((xcc + (unsigned)a) & (unsigned)(nq - 1));
            if (q_dry & (1u << q)) continue;
            const int pos = atomicAdd(qcnt + q * SORTED_QUEUE_STRIDE, 1);
            if (pos >= q_len) { q_dry |= 1u << q; continue; }
            got_y = pos / per_q;
            const int k = pos - got_y * per_q;
            int j0 = (homes[2 * got_y] - q + nq / 2) / nq;          // the queue's split nearest to the block's own
            j0 = j0 < 0 ? 0 : (j0 >= per_q ? per_q - 1 : j0);
            int j = (j0 + ((k & 1) ? (k + 1) / 2 : -(k / 2))) % per_q;
            if (j < 0) j += per_q;
            got = q + nq * j;
        }
        s_item[0] = got; s_item[1] = got_y; s_item[2] = (int)q_dry;
    }
    __syncthreads();
    split = __builtin_amdgcn_readfirstlane(s_item[0]); yblk = __builtin_amdgcn_readfirstlane(s_item[1]);   // (scalar registers, as blockIdx was)
    return split >= 0;                                              // (the whole workgroup: nothing left anywhere)
}

// Level 0v for ONE point and one block of GW groups (blk: its first group in the tfs tile): cm, the chunks of CG groups that
// can hold a vertex within thr1 of the point along v for this lane, from each chunk's two ends; todo, the wave's union.  2 fma, a
// max and a compare per chunk.  a_j = fma(0.5, -2qv_j, hv): the halving is exact, the one rounding is the subtraction's.  thr1
// only falls while levels 1-3 run, so a mask taken before them stays conservative.  n_in: the block's positions that hold a
// vertex; a block with padding at its tail (AV = 0 breaks the order) is not tested -- its chunks that hold a vertex pass.
template <int GW, int CG, typename cmask_t>
__device__ __forceinline__ void sorted_chunk_masks(const float4 *blk, int n_in, bool hit, float hv, float thr1, cmask_t &cm, cmask_t &todo)
{
    constexpr int NC = GW / CG;
    cm = 0; todo = 0;
    if (n_in >= 4 * GW) {
        // chunk c passes for this lane when the lane has this point in the block and the ends do not rule it out
        // (& rather than &&: no branch per chunk)
#define OA_VCHUNK_PASS(c, out)                                                                                                      \
        do {                                                                                                                        \
            const bool p_ = hit & !(out);                                                                                          \
            cm |= (cmask_t)p_ << (c);                                                                                              \
            if (__builtin_amdgcn_ballot_w64(p_)) todo |= (cmask_t)1 << (c);                                                         \
        } while (0)
        {                                                          // chunk 0: the block's position 0 on its own
            const float4 A0 = blk[1], A1 = blk[3 * (CG - 1) + 1];
            const float F = __builtin_fmaf(0.5f, A0.y, hv), L = __builtin_fmaf(0.5f, A1.w, hv);
            OA_VCHUNK_PASS(0, (__builtin_fmaxf(L, -F) > thr1) & (__builtin_fabsf(__builtin_fmaf(0.5f, A0.x, hv)) > thr1));
        }
#pragma unroll 5
        for (int c = 1; c < NC; ++c) {
            const float4 A0 = blk[3 * (CG * c) + 1], A1 = blk[3 * (CG * c + CG - 1) + 1];
            const float L = __builtin_fmaf(0.5f, A1.w, hv);
            if ((4 * GW > SORTED_VBLOCK) && (4 * CG * c) % SORTED_VBLOCK == 0) {   // (blocks of more than one: their 0s)
                const float F = __builtin_fmaf(0.5f, A0.y, hv);
                OA_VCHUNK_PASS(c, (__builtin_fmaxf(L, -F) > thr1) & (__builtin_fabsf(__builtin_fmaf(0.5f, A0.x, hv)) > thr1));
            } else {
                const float F = __builtin_fmaf(0.5f, A0.x, hv);
                OA_VCHUNK_PASS(c, __builtin_fmaxf(L, -F) > thr1);
            }
        }
#undef OA_VCHUNK_PASS
    } else {
#pragma unroll 1
        for (int c = 0; c < NC && 4 * CG * c < n_in; ++c) {
            cm |= (cmask_t)hit << c;
            todo |= (cmask_t)1 << c;
        }
    }
}

// The report: the item's bests into keys.  A split reports when it has something to say (k_nn_search_filtered); the seed's
// owner: seed index mod splits.  (The slot's index and the seed again from the record, instead of three registers per point
// held through the scan: the laundered index makes these loads new ones the compiler cannot merge with the prologue's, and
// that reload is what keeps the kernel at 0 B of scratch.)
template <int R>
__device__ __forceinline__ void sorted_report(const float4 *__restrict__ rec, int rec0, int ns_pad, unsigned long long *keys, int pass, int n_splits,
                                              int split, const float (&best)[R], const uint32_t (&bidx)[R])
{
    int rec1 = rec0;
    asm volatile("" : "+v"(rec1));
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(best[r]) << 32) | bidx[r];
        unsigned long long *dst = keys + __float_as_int(rec[rec1 + 64 * r].w);
        if (pass != 0) {                                           // merges into whatever keys holds: monotone
            if (key < __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(dst, key);
        } else if (n_splits == 1) *dst = key;
        else {
            const float4 rb = rec[ns_pad + rec1 + 64 * r];
            const float seed_d = rb.x;
            const uint32_t seed_idx = __float_as_uint(rb.y);
            const bool seeded = seed_idx != IDX_NONE;
            const bool improved = bidx[r] != seed_idx || best[r] != seed_d;
            const bool owner = seeded && (int)(seed_idx % (uint32_t)n_splits) == split;
            if (!seeded || improved || owner) atomicMin(dst, key);
        }
    }
}

// The kernel: per item (split, block of NN_THREADS x R source points) a scan of the split's tiles, double-buffered in LDS; per
// tile and block of GW groups level 0 for all the lane's points, and for a block some lane hit, point by point, level 0v and
// levels 1-3 (VCHUNK) or levels 1-3 for every group (not VCHUNK).  l0img: level 0's own images -- tmw or toct, as
// sorted_level0 says (launch_brute_sorted); not read by the per-vertex kind.
// pass 0: seeds from the winner records of the last accumulation (none on the first search of a loop: every split then has to
// find a best of its own before it can skip anything).  pass 2: seeds from keys, where k_nn_seed_sorted has left every point's
// nearest vertex within its own slab -- a distance really achieved, usually a few times the true one: enough for level 0.
template <int R, int TG = FTILE_GROUPS, bool VCHUNK = true>
__global__ __launch_bounds__(NN_THREADS, (R <= 4 ? 4 : 2)) void k_nn_search_sorted(const DevState *__restrict__ st,
                                                                 const float4 *__restrict__ tgs,
                                                                 const float4 *__restrict__ tfs,
                                                                 const float4 *__restrict__ tf3s,
                                                                 const int4 *__restrict__ tidx,
                                                                 int n_groups_pad,
                                                                 unsigned long long *keys, int pass,
                                                                 const float4 *__restrict__ rec,
                                                                 int n_splits, int n_blocks, const int *__restrict__ homes, int *qcnt,
                                                                 int nt, const float4 *__restrict__ l0img)
{
    if (st->halt) return;
    constexpr Level0 L0 = sorted_level0(R, VCHUNK);
    constexpr bool OWN_TILE = L0 != Level0::PerVertex;              // level 0 reads images of its own, staged beside the tfs tile
    constexpr bool POINT_PAIRS = level0_on_point_pairs(L0);
    constexpr bool IMAGES = L0 == Level0::Images;
    constexpr int TILE_F4 = TG * 3, LOADS = (TILE_F4 + NN_THREADS - 1) / NN_THREADS;   // TG = 256: 3 whole rounds; TG = 64: 192 of 256 threads
    constexpr bool WHOLE = TILE_F4 % NN_THREADS == 0;
    static_assert(LOADS >= 1 && LOADS <= 3, "k_nn_search_sorted: 1 .. 3 float4 per thread and tile");
    constexpr int TW = level0_tile_f4(L0, TG);                      // float4 of level 0's tile
    // a block: 4 GW = 256 vertices x R points per skip test.  Which blocks go on to level 1 is decided by the slabs' u, not by
    // the block size (256 sorted vertices of a million span 5e-4 of the axis, a point's reach 0.03), so larger blocks only save
    // compares, branches and waits for the tile: 16 / 32 / 64 / 128 / 256 / 512 vertices 31.1 / 28.8 / 28.0 / 27.6 / 27.3 /
    // 27.4 ms per iteration at 1M <-> 1M.  Folded 16 vertices (four images) at a time, fully unrolled (as a loop of four chunks
    // per trip: 28.3 ms).
    constexpr int GW = SORTED_GW < TG ? SORTED_GW : TG;
    static_assert(GW % 4 == 0 && TG % GW == 0, "k_nn_search_sorted: blocks of whole chunks of 16 vertices");
    static_assert(GW % SORTED_IMAGE_V == 0, "k_nn_search_sorted: blocks of whole trips of four images");
    // level 0v's chunks: CG groups each, NC per block; a lane's chunk bits in ONE register, the wave's union in a scalar
    constexpr int CG = SORTED_VCG, NC = GW / CG;
    static_assert(CG >= 1 && GW % CG == 0 && NC <= 64, "k_nn_search_sorted: level 0v's chunks");
    using cmask_t = typename std::conditional<(NC > 32), unsigned long long, uint32_t>::type;
    __shared__ float4 tile[2][TILE_F4];
    __shared__ float4 tilew[2][OWN_TILE ? TW : 1];
    __shared__ unsigned long long clk0[2];
    __shared__ int s_item[3];                                       // the workgroup's item {split, block}; [2]: the queues found empty so far
    const int tid0 = threadIdx.x;
    // qcnt == nullptr: one workgroup per (split, block), taken from the launch grid (n_splits = gridDim.x, n_blocks = gridDim.y)
    const bool queued = qcnt != nullptr;
    if (queued && tid0 == 0) s_item[2] = 0;
  for (;;) {
    // (the thread's index anew for every item: what is derived from it is then computed where it is used, as in the one-item form,
    //  instead of being hoisted out of this loop and held in registers -- or scratch -- through the scan)
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    int split = (int)blockIdx.x, yblk = (int)blockIdx.y;
    if (queued) {
        if (!sorted_take_item(tid, qcnt, homes, n_splits, n_blocks, s_item, split, yblk)) break;
    } else { n_splits = (int)gridDim.x; n_blocks = (int)gridDim.y; }
    const bool clk_wg = (split == 0 && yblk == n_blocks / 2 && tid == 0);   // one workgroup's item from the middle of the launch
    if (clk_wg) { clk0[0] = (unsigned long long)__builtin_readcyclecounter(); clk0[1] = wall_clock64(); }
    const double qmax = st->qmax;
    // a wave owns R x 64 CONSECUTIVE slots (neighbours in space: the smallest extent in u, the fewest slabs it must look into), and
    // so R x 64 consecutive records (k_sorted_point_setup, which also decides WHICH of the wave's slots a lane takes as its point
    // r): record rec0 + 64 r is point r of this lane -- coalesced loads, nothing to compute
    const int ns_pad = n_blocks * (NN_THREADS * R);
    const int rec0 = yblk * (NN_THREADS * R) + (tid >> 6) * (64 * R) + (tid & 63);
    // -- the lane's points from their records (written out: as a function it put <4, 256, false> into scratch).  co_find itself
    // (the record's third float4) is loaded where level 3 needs it: twelve registers (R = 4) not held through the scan --
    float hu[R], hv[R], hd[R], best[R], thr1[R], thr2[R];
    uint32_t bidx[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float4 ra = rec[rec0 + 64 * r], rb = rec[ns_pad + rec0 + 64 * r];
        hu[r] = ra.x; hv[r] = ra.y; hd[r] = ra.z;
        best[r] = rb.x; bidx[r] = __float_as_uint(rb.y); thr1[r] = rb.z; thr2[r] = rb.w;
        if (pass == 2) {
            // (the seed anew from keys, a 64-bit load: whatever another split has merged by now is as good.  keys only fall, so
            //  the key is the record's seed or beats it; the thresholds depend on the distance alone)
            const unsigned long long k = __hip_atomic_load(keys + __float_as_int(ra.w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float kd = __uint_as_float((uint32_t)(k >> 32));
            if ((uint32_t)k != IDX_NONE && kd < INFINITY && k < (((unsigned long long)__float_as_uint(best[r]) << 32) | bidx[r])) {
                const bool nearer = kd < best[r];
                best[r] = kd; bidx[r] = (uint32_t)k;
                if (nearer) sorted_thresholds(best[r], hu[r], hv[r], hd[r], qmax, thr1[r], thr2[r]);
            }
        }
    }
    // the lane's point pairs (2p, 2p + 1) for level 0: image from the set-up, the threshold from thr1 as it stands now
    float qhm[POINT_PAIRS ? R / 2 : 1], qhw[POINT_PAIRS ? R / 2 : 1], qthr[POINT_PAIRS ? R / 2 : 1];
    if constexpr (POINT_PAIRS) {
#pragma unroll
        for (int p = 0; p < R / 2; ++p) {
            const float4 rq = rec[3 * ns_pad + rec0 + 64 * p];
            qhm[p] = rq.x; qhw[p] = rq.y;
            qthr[p] = quad_threshold(thr1[2 * p], thr1[2 * p + 1], rq.z);
        }
    }

    int g_begin, g_end;
    split_range_of(split, n_splits, n_groups_pad, TG, g_begin, g_end);
    const int n_tiles = (g_end - g_begin) / TG;
    const float4 *tsrc = tfs + 3ll * g_begin;

    // visiting order of this split's tiles: middle-out from the tile that holds the u of the block's slot 0
    // (k_sorted_block_homes), or the split's end nearest to it -- tile_s, then tile_s + 1, tile_s - 1, ... for tile_m steps on
    // both sides, then the longer side alone; all of it scalar arithmetic, no loads beyond the block's home.  With seeds too: a
    // seed is the nearest vertex of the LAST pose, and the sooner the item meets the point's own slab, the sooner its thresholds
    // are final (seeded items in plain order: 25.1 against 24.0 ms per iteration at 1M <-> 1M, profiles/r10a_point_setup.txt).
    int tile_s = homes[2 * yblk + 1] - g_begin / TG;
    tile_s = tile_s < 0 ? 0 : (tile_s >= n_tiles ? n_tiles - 1 : tile_s);
    const bool tile_up = n_tiles - 1 - tile_s > tile_s;
    const int tile_m = tile_up ? tile_s : n_tiles - 1 - tile_s;
#define OA_TILE_AT(k) ((k) > 2 * tile_m ? (tile_up ? tile_s + (k) - tile_m : tile_s + tile_m - (k))                                  \
                                        : (((k) & 1) ? tile_s + (((k) + 1) >> 1) : tile_s - ((k) >> 1)))

    float4 stg0 = make_float4(0.f, 0.f, 0.f, 0.f), stg1 = stg0, stg2 = stg0, stgw = stg0;
    const float4 *wsrc = l0img + (IMAGES ? g_begin / SORTED_IMAGE_V * 3 : g_begin);  // (g_begin: a multiple of TG)
#define OA_STGW_ON (OWN_TILE && (TW >= NN_THREADS || tid < TW))
    static_assert(TW <= NN_THREADS && TG % 16 == 0, "k_nn_search_sorted: one float4 of level 0's images per thread and tile");
#define OA_STG_ON(k) (WHOLE || (k) * NN_THREADS + tid < TILE_F4)
#define OA_STG_EACH(OP)                                       \
    do {                                                      \
        if (LOADS > 0 && OA_STG_ON(0)) { OP(0, stg0); }       \
        if (LOADS > 1 && OA_STG_ON(1)) { OP(1, stg1); }       \
        if (LOADS > 2 && OA_STG_ON(2)) { OP(2, stg2); }       \
    } while (0)
    {
        const float4 *fsrc = tsrc + 3ll * TG * OA_TILE_AT(0);
#define OA_STG_FIRST(k, reg) reg = fsrc[(k) * NN_THREADS + tid]; tile[0][(k) * NN_THREADS + tid] = reg
        OA_STG_EACH(OA_STG_FIRST);
#undef OA_STG_FIRST
        if (OA_STGW_ON) { stgw = wsrc[TW * OA_TILE_AT(0) + tid]; tilew[0][tid] = stgw; }
    }
    __syncthreads();

    for (int t = 0; t < n_tiles; ++t) {
        const int cur = t & 1;
        const bool more = (t + 1 < n_tiles);
        if (more) {                                               // next tile: global -> registers, hidden under compute
            // (VCHUNK: the address from the scalar tile base and the thread's 32-bit offset, formed anew per tile -- held through
            //  the scan as a 64-bit vector pointer it is one register pair too many beside the larger rare path: scratch)
            const int nt1 = VCHUNK ? __builtin_amdgcn_readfirstlane(OA_TILE_AT(t + 1)) : OA_TILE_AT(t + 1);
            const float4 *nsrc = tsrc + 3ll * TG * nt1;
            int ltid = tid;
            if (VCHUNK) asm volatile("" : "+v"(ltid));
#define OA_STG_LOAD(k, reg) reg = nsrc[(k) * NN_THREADS + ltid]
            OA_STG_EACH(OA_STG_LOAD);
#undef OA_STG_LOAD
            if (OA_STGW_ON) stgw = wsrc[TW * nt1 + ltid];
        }
        const int gbase = g_begin + OA_TILE_AT(t) * TG;
        for (int g = 0; g < TG; g += GW) {
            const float4 *blk = &tile[cur][3 * g];                 // the block's groups in the tfs tile
            // level 0 (oa_level0.hpp): the block's smallest gap per point -- or point pair --, a trip of 16 vertices or four images
            // at a time, then ONE compare: can any of the lane's points not rule the whole block out?
            constexpr int NM = POINT_PAIRS ? R / 2 : R, TRIPS = IMAGES ? GW / SORTED_IMAGE_V : GW / 4;
            float m[NM], odd[NM];
#pragma unroll
            for (int c = 0; c < TRIPS; ++c) {
                if constexpr (L0 == Level0::PerVertex) {
                    // per vertex, from the tfs tile itself: |qu - hu|, one subtract and half a min3 per (vertex, point) pair, the |.| on
                    // the min's source modifier.  (Written out here: as a trip function like the point-pair kinds' it cost
                    // <4, 256, false> 12 B of scratch and <2, 256, false> a wave of occupancy.)
                    float4 QU[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) QU[k] = blk[3 * (4 * c + k)];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        float a[16];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            a[4 * k] = __builtin_fabsf(QU[k].x - hu[r]); a[4 * k + 1] = __builtin_fabsf(QU[k].y - hu[r]);
                            a[4 * k + 2] = __builtin_fabsf(QU[k].z - hu[r]); a[4 * k + 3] = __builtin_fabsf(QU[k].w - hu[r]);
                        }
                        level0_chain(a, c == 0, m[r], odd[r]);
                    }
                }
                else if constexpr (L0 == Level0::VertexPairs) {
                    // vertex pairs, per point: the pair images {m01, w01, m23, w23}, pair_gap -- per 16 vertices and point 16 subtracts
                    // (8 with |.| on their first source) and 4 min3.  (Written out as well: as a trip function the fold was
                    // scheduled differently and OA_NN_R=1 measured 29.05 -> 29.29 ms per step, outside the margin.)
                    float4 MW[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) MW[k] = tilew[cur][g + 4 * c + k];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        float a[8];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            a[2 * k] = pair_gap(MW[k].x, MW[k].y, hu[r]); a[2 * k + 1] = pair_gap(MW[k].z, MW[k].w, hu[r]);
                        }
                        level0_chain(a, c == 0, m[r], odd[r]);
                    }
                }
                else if constexpr (L0 == Level0::PointPairs) level0_point_pairs<R>(&tilew[cur][g + 4 * c], c == 0, qhm, qhw, m, odd);
                else level0_images<R>(&tilew[cur][3 * (g / SORTED_IMAGE_V + c)], c == 0, qhm, qhw, m, odd);
            }
            bool hit[R], hit0;
            if constexpr (POINT_PAIRS) hit0 = level0_pair_hits<R>(m, odd, qthr, hit);
            else {                                                 // per point (a NaN is a hit)
                hit0 = false;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    hit[r] = !(__builtin_fminf(m[r], odd[r]) > thr1[r]);
                    hit0 |= hit[r];
                }
            }
            if (!hit0) continue;
            if constexpr (POINT_PAIRS) {
                // the points' own coordinates from their records again, through a laundered index: the scan itself needs only
                // the pairs' images, and 3 R registers held through it for the rare path's sake are what pushed <4, 256, true>
                // into scratch
                int rh = rec0;
                asm volatile("" : "+v"(rh));
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float4 ra = rec[rh + 64 * r];
                    hu[r] = ra.x; hv[r] = ra.y; hd[r] = ra.z;
                }
            }
            if constexpr (VCHUNK) {
                // One point r at a time (the order in which groups are scored cannot change a lexicographic minimum): level 0v's
                // masks, then levels 1-3 for the chunks of the wave's.  (All R masks kept at once and a group-major loop cost
                // registers enough to spill the next tile's staging registers.)
                const int blk0 = __builtin_amdgcn_readfirstlane(gbase + g);   // the block's first group
                const int n_in = nt - 4 * blk0;                    // positions of the block that hold a vertex (when < 4 GW)
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (!__ballot(hit[r])) continue;               // (uniform: no lane of the wave has this point in the block)
                    cmask_t cm, todo;
                    sorted_chunk_masks<GW, CG, cmask_t>(blk, n_in, hit[r], hv[r], thr1[r], cm, todo);
                    for (; todo; todo &= todo - 1) {
                        // (todo is the wave's: made of ballots.  Said so, the chunk's tile addresses are scalar arithmetic)
                        const int c = __builtin_amdgcn_readfirstlane((NC > 32) ? __builtin_ctzll((unsigned long long)todo) : __builtin_ctz((uint32_t)todo));
                        const bool mine = (cm >> c) & 1;
                        // -- levels 1-3 for this point and chunk c (written out: as a function it adds a v_cmp_f32 per point) --
                        // Level 1 for the chunk's 4 CG vertices in one pass -- its 3 CG tile reads issued together and consumed in
                        // their order (the compiler counts the waits down, lgkmcnt(9) .. (0), but opens with a full one: a scalar
                        // load of level 2 may be pending on the back edge), the CG group minima kept, ONE test of their minimum per
                        // lane and one branch per chunk; only a chunk some lane still wants is walked group by group, a lane
                        // entering level 2 for a group whose stored minimum is not above its thr2 AS IT STANDS THEN (thr2 only
                        // falls, at level 3): the same groups reach level 2 as when each is scored on its own trip.  (One
                        // difference, which no answer can see: a group whose four scores are all NaN -- four non-finite vertices --
                        // does not carry its chunk past the test when the other groups' scores are numbers; such vertices never
                        // win.  A non-finite POINT makes every score NaN and passes everything.)
                        static_assert(CG >= 2 && CG <= 4, "k_nn_search_sorted: a chunk is 2-4 groups (their minima are held in registers)");
                        const float4 *cg = &tile[cur][3 * (g + CG * c)];
                        float4 Q[CG], AV[CG], W2[CG];
#pragma unroll
                        for (int k = 0; k < CG; ++k) { Q[k] = cg[3 * k]; AV[k] = cg[3 * k + 1]; W2[k] = cg[3 * k + 2]; }
                        float gmin[CG];
#pragma unroll
                        for (int k = 0; k < CG; ++k)
                            gmin[k] = sorted_level1_min(make_float4(-2.0f * Q[k].x, -2.0f * Q[k].y, -2.0f * Q[k].z, -2.0f * Q[k].w), AV[k], W2[k],
                                                        hu[r], hv[r]);
                        float cmin = gmin[0];
#pragma unroll
                        for (int k = 1; k < CG; ++k) cmin = __builtin_fminf(cmin, gmin[k]);   // v_min3_f32 (+ v_min_f32)
                        const bool want = mine & !(cmin > thr2[r]);
                        if (!__ballot(want)) continue;
                        // (the minima rotate through gmin[0] and the group's images come from the tile again: a loop of one copy of
                        //  levels 2-3 per point, and no register held for them through level 1)
#pragma unroll 1
                        for (int k = 0; k < CG; ++k) {
                            if (want && !(gmin[0] > thr2[r])) {
                                // (the point through laundered copies: what levels 2-3 derive from it alone -- the double precision
                                //  terms of the thresholds, a square root among them -- is then computed where a lane needs it,
                                //  not ahead of this loop for every block and point, and held in registers)
                                float lu = hu[r], lv = hv[r], ld = hd[r];
                                asm volatile("" : "+v"(lu), "+v"(lv), "+v"(ld));
                                const float4 Qk = cg[3 * k], AVk = cg[3 * k + 1];
                                sorted_finish_level2(make_float4(-2.0f * Qk.x, -2.0f * Qk.y, -2.0f * Qk.z, -2.0f * Qk.w), AVk, gbase + g + CG * c + k,
                                                     tf3s, tgs, tidx, rec + 2 * ns_pad + rec0 + 64 * r, lu, lv, ld, qmax, best[r], bidx[r],
                                                     thr1[r], thr2[r]);
                            }
#pragma unroll
                            for (int j = 0; j + 1 < CG; ++j) gmin[j] = gmin[j + 1];
                        }
                    }
                }
                if constexpr (POINT_PAIRS) {
                    // thr1 may have fallen: the point pairs' thresholds anew (the allowance again from the set-up's record, through
                    // a laundered index, instead of a register per pair held through the scan)
                    int rq = rec0;
                    asm volatile("" : "+v"(rq));
#pragma unroll
                    for (int p = 0; p < R / 2; ++p) qthr[p] = quad_threshold(thr1[2 * p], thr1[2 * p + 1], rec[3 * ns_pad + rq + 64 * p].z);
                }
            } else {                                               // OA_NN_VCHUNK=0: levels 1-3 for every group of the block
#pragma unroll 1
                for (int k = 0; k < GW; ++k) {                     // rare from here on: one group of 4 targets at a time
                    const float4 Q = tile[cur][3 * (g + k)], AV = tile[cur][3 * (g + k) + 1], W2 = tile[cur][3 * (g + k) + 2];
                    const float4 AU = make_float4(-2.0f * Q.x, -2.0f * Q.y, -2.0f * Q.z, -2.0f * Q.w);   // exact
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (!hit[r]) continue;                     // (a point's run of 64 slots is a quarter of the wave's extent)
                        sorted_finish_group(AU, AV, W2, gbase + g + k, tf3s, tgs, tidx, rec + 2 * ns_pad + rec0 + 64 * r, hu[r], hv[r], hd[r], qmax,
                                            best[r], bidx[r], thr1[r], thr2[r]);
                    }
                }
            }
        }
        if (more) {
#define OA_STG_STORE(k, reg) tile[cur ^ 1][(k) * NN_THREADS + tid] = reg
            OA_STG_EACH(OA_STG_STORE);
#undef OA_STG_STORE
            if (OA_STGW_ON) tilew[cur ^ 1][tid] = stgw;
        }
        __syncthreads();
    }
#undef OA_STG_EACH
#undef OA_STG_ON
#undef OA_STGW_ON
#undef OA_TILE_AT

    if (clk_wg) {
        DevState *ws = const_cast<DevState *>(st);
        ws->search_clk[0] = (unsigned long long)__builtin_readcyclecounter() - clk0[0];
        ws->search_clk[1] = wall_clock64() - clk0[1];
    }
    sorted_report<R>(rec, rec0, ns_pad, keys, pass, n_splits, split, best, bidx);
    if (!queued) break;
  }
}

// ------------------------------------------------------------------------------------------------
// k_pair_accumulate
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Optional normal-angle rejection (an EXTENSION: the reference has no such test -- SURVEY.md D3).  A pair is kept
// only if the angle between the world-space normals of the source vertex and of its correspondence is at most
// max_angle.  Normals are carried to world space with the inverse-transpose of the object matrices (imx1 / imx2).
struct NormalTest {
    const float *src_n;     // ns x 3, align-local, same slot order as src4 (nullptr = test disabled)
    const float *tgt_n;     // nt x 3 per target vertex (vertex mode); nullptr in surface mode = geometric face normal
    double cos_min;
};
// ... and, for the kernels that open with pair_fetch, the reciprocal check's verdict beside it (oa_set_reciprocal, oa_recip.hpp:
// k_recip_check): one byte per slot, 0 = the pair is not mutual.  A COMPILE-TIME switch, not a nullable pointer in NormalTest: the
// extra pointer cost k_pair_accumulate_canon, _plane<false> and k_residual_keys<true> two VGPRs each (and _plane<false> a wave of
// occupancy) with the check off.  PairTest<false> IS NormalTest: the kernels<.., false> are the ones from before the check.
struct NormalTestRecip : NormalTest {
    const unsigned char *recip_ok;
};
template <bool RECIP> using PairTest = std::conditional_t<RECIP, NormalTestRecip, NormalTest>;

__device__ __forceinline__ bool normal_angle_ok(const float *imx1, const float *imx2, const float *ns, const float *nt,
                                                double cos_min)
{
    double a[3], b[3];
    for (int k = 0; k < 3; ++k) {      // (M^-1)^T n : column k of the inverse dotted with n
        a[k] = (double)imx1[k] * (double)ns[0] + (double)imx1[4 + k] * (double)ns[1] + (double)imx1[8 + k] * (double)ns[2];
        b[k] = (double)imx2[k] * (double)nt[0] + (double)imx2[4 + k] * (double)nt[1] + (double)imx2[8 + k] * (double)nt[2];
    }
    const double ab = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    const double aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    const double bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    const double c = ab / sqrt(aa * bb);
    return c >= cos_min;               // NaN (zero normal) -> rejected
}

// Wave-level sum of the 24 running sums: a reduce-scatter butterfly.  Each exchange step halves the number of values
// a lane still carries (24 -> 12 -> 6 -> 3, partner = lane ^ 32, ^ 16, ^ 8), then the remaining 3 values are summed
// over the 8 lanes that share bits 5..3 (^ 4, ^ 2, ^ 1): 30 double shuffles instead of 24 x 6 = 144.  Afterwards every
// lane holds, in out[0..2], the wave totals of sums number first .. first + 2.  Fixed pattern => bitwise reproducible.
__device__ __forceinline__ void wave_reduce_sums(const double (&acc)[NSUMS], int lane, double (&out)[3], int &first)
{
    double a12[12], a6[6];
    const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const double keep = b5 ? acc[12 + k] : acc[k], send = b5 ? acc[k] : acc[12 + k];
        a12[k] = keep + __shfl_xor(send, 32, 64);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double keep = b4 ? a12[6 + k] : a12[k], send = b4 ? a12[k] : a12[6 + k];
        a6[k] = keep + __shfl_xor(send, 16, 64);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double keep = b3 ? a6[3 + k] : a6[k], send = b3 ? a6[k] : a6[3 + k];
        double v = keep + __shfl_xor(send, 8, 64);
        v += __shfl_xor(v, 4, 64);
        v += __shfl_xor(v, 2, 64);
        v += __shfl_xor(v, 1, 64);
        out[k] = v;
    }
    first = (b5 ? 12 : 0) + (b4 ? 6 : 0) + (b3 ? 3 : 0);
}

struct PairOut {            // optional per-point outputs for the make_pairs contract
    unsigned char *valid;   // ns
    float  *b;              // ns x 3  (imx1 @ (mx2 @ co1))
    double *dist;           // ns
    int    *nn_idx;         // ns
    float  *nn_d2;          // ns
    const int *perm;        // sorted slot -> caller-order slot (nullptr = identity); outputs are in caller order
};

// ---- the pair test and its contribution to the sums: shared by k_pair_accumulate and by the search kernels that
// accumulate in their epilogue (same operations, same order, same bits) ------------------------------------------------
// (cx, cy, cz) = co_find, the source point in base-local space; (qx, qy, qz) = co1, its correspondence there;
// tn = the correspondence's normal (only read when the normal-angle extension is on); slot = the source slot (normals).
// Returns the reference's `dist < thresh` (functions/general.py:299-302) and, for a pair that passes, b = imx1 @ (mx2 @ co1).
__device__ __forceinline__ bool pair_eval(const DevState *__restrict__ st, float cx, float cy, float cz, float qx, float qy,
                                          float qz, const NormalTest &nrm, long long slot, const float *tn, double thresh,
                                          float &bx, float &by, float &bz, double &dist)
{
    float ax = cx, ay = cy, az = cz, wbx = qx, wby = qy, wbz = qz;
    if (!st->mx2_identity) {
        // (with the identity the products below return their argument bit for bit -- up to the sign of a zero, which neither
        //  the distance nor b can see -- and the two of them are a fifth of this function's fp64 work)
        m4_mul_v3(st->mx2, cx, cy, cz, ax, ay, az);     // mx2 @ co_find             (general.py:299)
        m4_mul_v3(st->mx2, qx, qy, qz, wbx, wby, wbz);  // mx2 @ co1                 (general.py:299)
    }
    dist = v3_length(ax - wbx, ay - wby, az - wbz);
    bool valid = dist < thresh;                        // face_index != -1 always holds (general.py:302)
    if (valid && nrm.src_n) {
        const float sn[3] = { nrm.src_n[3ll * slot], nrm.src_n[3ll * slot + 1], nrm.src_n[3ll * slot + 2] };
        valid = normal_angle_ok(st->imx1, st->imx2, sn, tn, nrm.cos_min);
    }
    bx = by = bz = 0.f;
    if (valid) m4_mul_v3(st->imx1, wbx, wby, wbz, bx, by, bz);   // imx1 @ (mx2 @ co1)  (general.py:304)
    return valid;
}

// ---- the per-slot correspondence fetch: what "the same pair" means for every stand-alone accumulation kernel and for
// k_residual_keys.  Slot i's search result keys[i] (distance bits << 32 | index) -> co_find = the source point in base-local
// space (general.py:287) -> co1 = its correspondence there (general.py:297) and that correspondence's normal tn -> pair_eval.
//   surface mode (tri9):  co1 = the closest point on triangle idx; tn = the geometric face normal, in the operand order of
//                         Blender's normal_tri_v3 (cross(a - b, b - c), not normalised).
//   vertex mode:          co1 = target vertex idx, from the slot's winner record (coordinates + index) when its index matches,
//                         else gathered from tgt_xyz.  The grid and tree searches leave this search's winner in the record;
//                         after a brute-force search it still holds the previous winner, which in a converging loop is mostly
//                         the same vertex.  win == nullptr: no records (surface mode), every slot gathers.
// The two switches are the ONLY differences between the callers:
//   WRITES    true  (the accumulating kernels): keys[i] is reset to KEY_EMPTY for the next iteration's atomicMin, prev[i]
//                   (if given) takes the index as the seed of the next filtered search, a record that missed is rewritten.
//             false (k_residual_keys): keys, prev and win stay as the search left them; prev is not read at all.
//   METRIC_N  false (point metric): tn is read by the normal-angle test alone -- nrm.tgt_n[idx] resp. the face normal when
//                   nrm.src_n is set, zeros otherwise.
//             true  (plane, GICP): tn is the metric's normal -- plane_tn[idx] resp. the face normal, always.
// f.p is loaded before the IDX_NONE test (the callers use it for a slot without a pair too); a slot without a pair leaves
// tn, b and dist zero.  Returns pair_eval's verdict -- and, RECIP, false for a slot the reciprocal check rejected
// (nrm.recip_ok[i] == 0), after everything above: the WRITES side effects are the same, so seeds survive a rejection.
struct PairFetch {
    float4 p;                   // src4[i]
    unsigned long long key;     // keys[i] as the search left it
    uint32_t idx;               // its index part (IDX_NONE: no candidate)
    float tn[3];                // the correspondence's normal, base-local
    float bx, by, bz;           // imx1 @ (mx2 @ co1)
    double dist;                // the world-space pair distance
};

template <bool WRITES, bool METRIC_N, bool RECIP = false>
__device__ __forceinline__ bool pair_fetch(const DevState *__restrict__ st, const float4 *__restrict__ src4, int i,
                                           const float *__restrict__ tgt_xyz,
                                           std::conditional_t<WRITES, unsigned long long, const unsigned long long> *__restrict__ keys,
                                           int *__restrict__ prev, std::conditional_t<WRITES, float4, const float4> *__restrict__ win,
                                           const float4 *__restrict__ tri9, const PairTest<RECIP> &nrm,
                                           const float *__restrict__ plane_tn, double thresh, PairFetch &f)
{
    f.key = keys[i];
    if constexpr (WRITES) keys[i] = KEY_EMPTY;
    const uint32_t idx = f.idx = (uint32_t)f.key;
    if constexpr (WRITES) { if (prev) prev[i] = (idx == IDX_NONE) ? -1 : (int)idx; }
    f.bx = f.by = f.bz = 0.f;
    f.dist = 0.0;
    f.tn[0] = f.tn[1] = f.tn[2] = 0.f;
    f.p = src4[i];
    float4 wrec = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    if (win) wrec = win[i];
    if (idx == IDX_NONE) return false;
    float cx, cy, cz;
    co_find(st, f.p.x, f.p.y, f.p.z, cx, cy, cz);
    float qx, qy, qz;
    if (tri9) {
        float ta[3], tb[3], tc[3], rr[3];
        const float cf[3] = { cx, cy, cz };
        load_tri(tri9, idx, ta, tb, tc);
        closest_on_tri(cf, ta, tb, tc, rr);
        qx = rr[0]; qy = rr[1]; qz = rr[2];
        if (METRIC_N || nrm.src_n) {
            const float e1[3] = { ta[0] - tb[0], ta[1] - tb[1], ta[2] - tb[2] };
            const float e2[3] = { tb[0] - tc[0], tb[1] - tc[1], tb[2] - tc[2] };
            f.tn[0] = e1[1] * e2[2] - e1[2] * e2[1];
            f.tn[1] = e1[2] * e2[0] - e1[0] * e2[2];
            f.tn[2] = e1[0] * e2[1] - e1[1] * e2[0];
        }
    } else {
        if ((uint32_t)__float_as_int(wrec.w) == idx) { qx = wrec.x; qy = wrec.y; qz = wrec.z; }
        else {
            qx = tgt_xyz[3ll * idx]; qy = tgt_xyz[3ll * idx + 1]; qz = tgt_xyz[3ll * idx + 2];
            if constexpr (WRITES) { if (win) win[i] = make_float4(qx, qy, qz, __int_as_float((int)idx)); }
        }
        if constexpr (METRIC_N) { f.tn[0] = plane_tn[3ll * idx]; f.tn[1] = plane_tn[3ll * idx + 1]; f.tn[2] = plane_tn[3ll * idx + 2]; }
        else if (nrm.src_n) { f.tn[0] = nrm.tgt_n[3ll * idx]; f.tn[1] = nrm.tgt_n[3ll * idx + 1]; f.tn[2] = nrm.tgt_n[3ll * idx + 2]; }
    }
    const bool valid = pair_eval(st, cx, cy, cz, qx, qy, qz, nrm, i, f.tn, thresh, f.bx, f.by, f.bz, f.dist);
    if constexpr (RECIP) return valid && nrm.recip_ok[i] != 0;
    else return valid;
}

__device__ __forceinline__ void pair_add(double (&acc)[NSUMS], float p_x, float p_y, float p_z, float bx, float by, float bz,
                                         double dist, double pvx, double pvy, double pvz, double d_pivot)
{
    const double a0 = (double)p_x - pvx, a1 = (double)p_y - pvy, a2 = (double)p_z - pvz;
    const double b0 = (double)bx - pvx, b1 = (double)by - pvy, b2 = (double)bz - pvz;
    acc[S_A] += a0; acc[S_A + 1] += a1; acc[S_A + 2] += a2;
    acc[S_B] += b0; acc[S_B + 1] += b1; acc[S_B + 2] += b2;
    acc[S_H + 0] += b0 * a0; acc[S_H + 1] += b0 * a1; acc[S_H + 2] += b0 * a2;
    acc[S_H + 3] += b1 * a0; acc[S_H + 4] += b1 * a1; acc[S_H + 5] += b1 * a2;
    acc[S_H + 6] += b2 * a0; acc[S_H + 7] += b2 * a1; acc[S_H + 8] += b2 * a2;
    acc[S_AA] += (a0 * a0 + a1 * a1) + a2 * a2;
    acc[S_BB] += (b0 * b0 + b1 * b1) + b2 * b2;
    acc[S_K] += 1.0;
    const double dd = dist - d_pivot;
    acc[S_D] += dd;
    acc[S_DD] += dd * dd;
}

// every lane's acc -> the workgroup's totals -> one row of per-workgroup partials (wave butterfly, then the waves in
// order through LDS: a fixed pattern, bitwise reproducible).  red: __shared__ double[blockDim.x / 64][NSUMS].
// Called by ALL threads of the workgroup.
__device__ __forceinline__ void block_store_partial(const double (&acc)[NSUMS], double (*red)[NSUMS], double *__restrict__ row)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {
        double tot[3];
        int first;
        wave_reduce_sums(acc, lane, tot, first);
        if ((lane & 7) == 0) { red[wave][first] = tot[0]; red[wave][first + 1] = tot[1]; red[wave][first + 2] = tot[2]; }
    }
    __syncthreads();
    if (threadIdx.x < NSUMS) {
        double v = red[0][threadIdx.x];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) v += red[w][threadIdx.x];
        row[threadIdx.x] = v;
    }
}

// The same for search kernels whose lanes hold ONE pair each (k_nn_search_grid<L, true>): the 20 sums are formed and
// reduced in two halves of 12 and 8, so that the epilogue of a kernel built for 6 waves per SIMD (80 VGPRs) never holds 24
// doubles plus the butterfly's temporaries at once.  Reduce-scatter over lane bits 5, 4 (, 3), then a plain butterfly.
// (a, b) = the pair relative to the pivot, dd = dist - d_pivot; lanes without a valid pair contribute zeros.
// The exchanges stay in the VALU (round 3; they were ds_bpermute pairs with a select on either side -- 62 LDS operations and
// as many selects per wave): gfx950's v_permlane32_swap / v_permlane16_swap ARE the halving step (the upper half of one
// register against the lower half of the other: each half keeps its value and receives the other half's copy of it), and the
// butterflies inside a row of 16 lanes are DPP moves.  Same additions between the same values as before (operands swapped in
// half of the lanes; IEEE addition commutes), so the rows keep their bits: tools/reduce_check.hip holds the old form.
__device__ __forceinline__ double f64_from(unsigned lo, unsigned hi) { return __hiloint2double((int)hi, (int)lo); }

// lanes 0..31: a[l] + a[l + 32]     lanes 32..63: b[l - 32] + b[l]
__device__ __forceinline__ double halve_add32(double a, double b)
{
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    return f64_from(lo[0], hi[0]) + f64_from(lo[1], hi[1]);
}

// even rows of 16 lanes: a[l] + a[l + 16]     odd rows: b[l - 16] + b[l]
__device__ __forceinline__ double halve_add16(double a, double b)
{
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    return f64_from(lo[0], hi[0]) + f64_from(lo[1], hi[1]);
}

// t[l ^ X] inside a row of 16 lanes: X = 8 is a rotation by 8, X = 2 and 1 are quad permutations; X = 4 takes lane l + 4 in
// the banks {0..3, 8..11} and lane l - 4 in the others (two DPP moves into one register)
template <int X>
__device__ __forceinline__ double row_xor(double t)
{
    static_assert(X == 8 || X == 4 || X == 2 || X == 1, "");
    const int lo = __double2loint(t), hi = __double2hiint(t);
    int rl, rh;
    if (X == 4) {
        rl = __builtin_amdgcn_update_dpp(lo, lo, 0x104, 0xf, 0x5, false);      // row_shl:4 -> banks 0, 2
        rl = __builtin_amdgcn_update_dpp(rl, lo, 0x114, 0xf, 0xa, false);      // row_shr:4 -> banks 1, 3
        rh = __builtin_amdgcn_update_dpp(hi, hi, 0x104, 0xf, 0x5, false);
        rh = __builtin_amdgcn_update_dpp(rh, hi, 0x114, 0xf, 0xa, false);
    } else {
        constexpr int ctrl = X == 8 ? 0x128 : (X == 2 ? 0x4e : 0xb1);           // row_ror:8, quad_perm [2,3,0,1], [1,0,3,2]
        rl = __builtin_amdgcn_update_dpp(lo, lo, ctrl, 0xf, 0xf, false);
        rh = __builtin_amdgcn_update_dpp(hi, hi, ctrl, 0xf, 0xf, false);
    }
    return __hiloint2double(rh, rl);
}

template <int N>
__device__ __forceinline__ void wave_reduce_scatter(double (&v)[N], int lane, double *red_row)
{
    static_assert(N == 12 || N == 8, "halves of the 24 sums");
    const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0;
    double u[N / 2], w[3];                                          // (w: N / 4 values; 3 slots so that the N == 12 branch indexes in bounds when N == 8 is compiled)
#pragma unroll
    for (int k = 0; k < N / 2; ++k) u[k] = halve_add32(v[k], v[N / 2 + k]);     // lower half of the wave: v[k], upper: v[N/2 + k]
#pragma unroll
    for (int k = 0; k < N / 4; ++k) w[k] = halve_add16(u[k], u[N / 4 + k]);
    if (N == 12) {                                                   // 3 values left, 16 lanes share them
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double t = w[k];
            t += row_xor<8>(t); t += row_xor<4>(t); t += row_xor<2>(t); t += row_xor<1>(t);
            w[k] = t;
        }
        if ((lane & 15) == 0) {
            const int first = (b5 ? 6 : 0) + (b4 ? 3 : 0);
            red_row[first] = w[0]; red_row[first + 1] = w[1]; red_row[first + 2] = w[2];
        }
    } else {                                                         // 2 values left: one more halving, then 8 lanes share one
        const double keep = b3 ? w[1] : w[0], send = b3 ? w[0] : w[1];
        double t = keep + row_xor<8>(send);
        t += row_xor<4>(t); t += row_xor<2>(t); t += row_xor<1>(t);
        if ((lane & 7) == 0) red_row[(b5 ? 4 : 0) + (b4 ? 2 : 0) + (b3 ? 1 : 0)] = t;
    }
}

// red: __shared__ double[blockDim.x / 64][NSUMS].  Called by ALL threads of the workgroup.
// (Combining the workgroups' rows any further inside the launch -- groups of 16 meeting at a counter, rows and counter in
// agent-scope atomics -- was built and measured: the store -> acknowledge -> atomic -> load chain adds 4-5 us to the end
// of every launch, more than the wider reduction it saves; a reduction over several workgroups meeting at ONE counter
// costs +8 us with 16 of them and +16..23 us with 64, with or without fences.  So: one row per workgroup, one wide
// single-workgroup reduction behind it.)
__device__ __forceinline__ void block_store_pair(bool valid, double a0, double a1, double a2, double b0, double b1, double b2,
                                                 double dd, double (*red)[NSUMS], double *__restrict__ row,
                                                 long long *stamps = nullptr)      // instrumented builds: clock after the wave's part, after the barrier
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (!valid) { a0 = a1 = a2 = b0 = b1 = b2 = dd = 0.0; }
    {
        double h[12] = { a0, a1, a2, b0, b1, b2, b0 * a0, b0 * a1, b0 * a2, b1 * a0, b1 * a1, b1 * a2 };   // sums 0 .. 11
        wave_reduce_scatter<12>(h, lane, &red[wave][0]);
    }
    {
        double h[8] = { b2 * a0, b2 * a1, b2 * a2, (a0 * a0 + a1 * a1) + a2 * a2, (b0 * b0 + b1 * b1) + b2 * b2,
                        valid ? 1.0 : 0.0, dd, dd * dd };                                                       // sums 12 .. 19
        wave_reduce_scatter<8>(h, lane, &red[wave][12]);
    }
    if (lane < 4) red[wave][20 + lane] = 0.0;                                                                   // reserved
    if (stamps) stamps[0] = (long long)__builtin_readcyclecounter();
    __syncthreads();
    if (stamps) stamps[1] = (long long)__builtin_readcyclecounter();
    if (threadIdx.x < NSUMS) {
        double v = red[0][threadIdx.x];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) v += red[w][threadIdx.x];
        row[threadIdx.x] = v;
    }
}

template <bool EMIT, bool RECIP = false>
__global__ __launch_bounds__(ACC_THREADS) void k_pair_accumulate(const DevState *__restrict__ st,
                                                                 const float4 *__restrict__ src4, int ns,
                                                                 const float *__restrict__ tgt_xyz,
                                                                 unsigned long long *__restrict__ keys,
                                                                 int *__restrict__ prev, float4 *__restrict__ win,
                                                                 const float4 *__restrict__ tri9, PairTest<RECIP> nrm,
                                                                 double *__restrict__ partials, PairOut out,
                                                                 unsigned long long *__restrict__ t_acc_start)
{
    __shared__ double red[ACC_THREADS / 64][NSUMS];
    if (t_acc_start && blockIdx.x == 0 && threadIdx.x == 0) *t_acc_start = wall_clock64();   // ~ the end of the search
    double acc[NSUMS];
#pragma unroll
    for (int k = 0; k < NSUMS; ++k) acc[k] = 0.0;
    const bool halted = st->halt != 0;
    const double thresh = st->thresh;
    const double pvx = st->pivot[0], pvy = st->pivot[1], pvz = st->pivot[2];
    const double d_pivot = st->d_pivot;

    if (!halted) {
        for (int i = blockIdx.x * ACC_THREADS + threadIdx.x; i < ns; i += gridDim.x * ACC_THREADS) {
            PairFetch f;
            const bool valid = pair_fetch<true, false, RECIP>(st, src4, i, tgt_xyz, keys, prev, win, tri9, nrm, nullptr, thresh, f);
            if (EMIT) {
                const long long o = out.perm ? out.perm[i] : i;
                out.valid[o] = valid ? 1 : 0;
                out.b[3 * o] = f.bx; out.b[3 * o + 1] = f.by; out.b[3 * o + 2] = f.bz;
                out.dist[o] = f.dist;
                if (out.nn_idx) { out.nn_idx[o] = (int)f.idx; out.nn_d2[o] = __uint_as_float((uint32_t)(f.key >> 32)); }
            }
            if (valid) pair_add(acc, f.p.x, f.p.y, f.p.z, f.bx, f.by, f.bz, f.dist, pvx, pvy, pvz, d_pivot);
        }
    }
    block_store_partial(acc, red, partials + (long long)blockIdx.x * NSUMS);
}

// The stand-alone form of what k_nn_search_grid<L, true> does in its epilogue: one thread per (source slot, lane of the
// query), the same pair test, the same reduction tree, the same rows -- BIT FOR BIT.  The loop switches between "the grid
// search finishes and accumulates everything itself" and "grid search -> tree search of the hand-over list -> this kernel"
// from one iteration to the next on what the host last heard about the list (oa_icp.hip: adaptive path), and that choice
// depends on timing: it must not show in the sums.  The brute-force searches use it too (for shards whose rows fit), so
// every search mode still ends with bitwise the same matrices.
// Launched with the workgroup size the accumulating grid search of this shard uses (256 or 512 threads, oa_icp.hip:
// canon_threads): the same workgroups, hence the same rows.
constexpr int CANON_THREADS = 512;
// (RECIP: the variant behind k_recip_check, see PairTest; <false> is the kernel the fused searches are twins of)
template <bool RECIP = false>
__global__ __launch_bounds__(CANON_THREADS) void k_pair_accumulate_canon(const DevState *__restrict__ st, const float4 *__restrict__ src4,
                                                               int ns, const float *__restrict__ tgt_xyz,
                                                               unsigned long long *__restrict__ keys, int *__restrict__ prev,
                                                               float4 *__restrict__ win, const float4 *__restrict__ tri9,
                                                               PairTest<RECIP> nrm, int L, double *__restrict__ partials,
                                                               unsigned long long *__restrict__ t_acc_start)
{
    __shared__ double red[CANON_THREADS / 64][NSUMS];
    if (t_acc_start && blockIdx.x == 0 && threadIdx.x == 0) *t_acc_start = wall_clock64();   // ~ the end of the search
    if (st->halt) return;
    const int gt = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = gt / L;
    const bool mine = (gt - i * L) == 0 && i < ns;
    bool valid = false;
    PairFetch f = {};
    if (mine) valid = pair_fetch<true, false, RECIP>(st, src4, i, tgt_xyz, keys, prev, win, tri9, nrm, nullptr, st->thresh, f);
    const double pvx = st->pivot[0], pvy = st->pivot[1], pvz = st->pivot[2];
    block_store_pair(valid, (double)f.p.x - pvx, (double)f.p.y - pvy, (double)f.p.z - pvz, (double)f.bx - pvx, (double)f.by - pvy,
                     (double)f.bz - pvz, f.dist - st->d_pivot, red, partials + (long long)blockIdx.x * NSUMS);
}

// ---- weighted steps of the point metric (oa_set_robust / oa_set_source_weights) -----------------------------------------
// the wave's total of ONE value in every lane: the halving steps of wave_reduce_scatter with both operands the same register
// (each half receives the other half's copy), then the butterfly inside a row of 16 lanes.  Fixed pattern.
__device__ __forceinline__ double wave_sum_all(double t)
{
    t = halve_add32(t, t);
    t = halve_add16(t, t);
    t += row_xor<8>(t); t += row_xor<4>(t); t += row_xor<2>(t); t += row_xor<1>(t);
    return t;
}

// block_store_pair with a weight per pair: sums 0 .. 16 carry w, K and the distance sums do not, S_W = sum w.  The same two
// slices of 12 + 8 through the same reduce-scatter, and one more value.  red: __shared__ double[blockDim.x / 64][NSUMS].
__device__ __forceinline__ void block_store_pair_weighted(bool valid, double w, double a0, double a1, double a2, double b0, double b1,
                                                          double b2, double dd, double (*red)[NSUMS], double *__restrict__ row)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (!valid) { a0 = a1 = a2 = b0 = b1 = b2 = dd = w = 0.0; }
    const double wb0 = w * b0, wb1 = w * b1, wb2 = w * b2;
    {
        double h[12] = { w * a0, w * a1, w * a2, wb0, wb1, wb2, wb0 * a0, wb0 * a1, wb0 * a2, wb1 * a0, wb1 * a1, wb1 * a2 };   // sums 0 .. 11
        wave_reduce_scatter<12>(h, lane, &red[wave][0]);
    }
    {
        double h[8] = { wb2 * a0, wb2 * a1, wb2 * a2, w * ((a0 * a0 + a1 * a1) + a2 * a2), w * ((b0 * b0 + b1 * b1) + b2 * b2),
                        valid ? 1.0 : 0.0, dd, dd * dd };                                                           // sums 12 .. 19
        wave_reduce_scatter<8>(h, lane, &red[wave][12]);
    }
    const double wsum = wave_sum_all(w);
    if (lane < 4) red[wave][S_W + lane] = lane == 0 ? wsum : 0.0;                                                   // sum 20, reserved
    __syncthreads();
    if (threadIdx.x < NSUMS) {
        double v = red[0][threadIdx.x];
        for (int k = 1; k < (int)(blockDim.x >> 6); ++k) v += red[k][threadIdx.x];
        row[threadIdx.x] = v;
    }
}

// k_pair_accumulate_canon with a weight per pair: the same pair (pair_fetch<true, false>), ONE thread per source slot, the
// same fixed-order reduction (no float atomics).  w = w_vertex * psi(dist):
// dist = the world-space pair distance of pair_eval; w_slot = one weight per slot (nullptr: all 1); the loss and its scale are
// launch-uniform (DevState).  Its workgroups depend on the shard size alone, so every search mode leaves the same rows.
constexpr int WEIGHTED_THREADS = 512;
template <bool RECIP = false>
__global__ __launch_bounds__(WEIGHTED_THREADS) void k_pair_accumulate_weighted(const DevState *__restrict__ st, const float4 *__restrict__ src4,
                                                               int ns, const float *__restrict__ tgt_xyz,
                                                               unsigned long long *__restrict__ keys, int *__restrict__ prev,
                                                               float4 *__restrict__ win, const float4 *__restrict__ tri9,
                                                               PairTest<RECIP> nrm, const float *__restrict__ w_slot,
                                                               double *__restrict__ partials,
                                                               unsigned long long *__restrict__ t_acc_start)
{
    __shared__ double red[WEIGHTED_THREADS / 64][NSUMS];
    if (t_acc_start && blockIdx.x == 0 && threadIdx.x == 0) *t_acc_start = wall_clock64();   // ~ the end of the search
    if (st->halt) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = false;
    double w = 0.0;
    PairFetch f = {};
    if (i < ns) {
        valid = pair_fetch<true, false, RECIP>(st, src4, i, tgt_xyz, keys, prev, win, tri9, nrm, nullptr, st->thresh, f);
        if (valid) {
            w = robust_psi(st->loss, f.dist, st->robust_c);
            if (w_slot) w *= (double)w_slot[i];
        }
    }
    const double pvx = st->pivot[0], pvy = st->pivot[1], pvz = st->pivot[2];
    block_store_pair_weighted(valid, w, (double)f.p.x - pvx, (double)f.p.y - pvy, (double)f.p.z - pvz, (double)f.bx - pvx, (double)f.by - pvy,
                              (double)f.bz - pvz, f.dist - st->d_pivot, red, partials + (long long)blockIdx.x * NSUMS);
}

// ---- the point-to-plane metric (oa_set_metric(OA_METRIC_PLANE)): the same pair test, the sums of the plane system ---------
// The correspondence's normal in align-local space, unit length, fp64: base-local tn -> world with the inverse transpose of
// mx2 (as normal_angle_ok carries it) -> align-local with mx1^T (the inverse transpose of imx1).  false: zero or non-finite
// length (a degenerate triangle) -- the pair then takes no part in the step.
__device__ __forceinline__ bool plane_normal(const DevState *__restrict__ st, const float *tn, double &nx, double &ny, double &nz)
{
    double w[3], l[3];
    for (int k = 0; k < 3; ++k)
        w[k] = (double)st->imx2[k] * (double)tn[0] + (double)st->imx2[4 + k] * (double)tn[1] + (double)st->imx2[8 + k] * (double)tn[2];
    for (int k = 0; k < 3; ++k)
        l[k] = (double)st->mx1[k] * w[0] + (double)st->mx1[4 + k] * w[1] + (double)st->mx1[8 + k] * w[2];
    const double n2 = (l[0] * l[0] + l[1] * l[1]) + l[2] * l[2];
    if (!(n2 > 0.0) || !(n2 < INFINITY)) return false;
    const double inv = 1.0 / sqrt(n2);
    nx = l[0] * inv; ny = l[1] * inv; nz = l[2] * inv;
    return true;
}

// residual and Jacobian row of one pair (a, b relative to the pivot; n unit)
__device__ __forceinline__ void plane_row(double a0, double a1, double a2, double b0, double b1, double b2, double nx, double ny, double nz,
                                          double (&j)[6], double &r)
{
    r = (nx * (a0 - b0) + ny * (a1 - b1)) + nz * (a2 - b2);
    j[0] = a1 * nz - a2 * ny; j[1] = a2 * nx - a0 * nz; j[2] = a0 * ny - a1 * nx;
    j[3] = nx; j[4] = ny; j[5] = nz;
}

// The symmetric metric's row (OA_METRIC_SYMMETRIC; Rusinkiewicz, "A Symmetric Objective Function for ICP", 2019): plane_row's
// shape -- rank one -- with n = (n_b + s n_a) / 2, s = the sign of n_a . n_b (left-to-right sum, an exact 0 counts as +1), and
// the lever arm a + b.  na, nb unit.  |n|^2 = (1 + |cos|) / 2 >= 1/2: never zero.  Flipping n_a leaves n the same bits
// (s flips with it); flipping n_b flips n, j and r together, so no product j j^T, j r moves.
__device__ __forceinline__ void symm_row(double a0, double a1, double a2, double b0, double b1, double b2, double ax, double ay, double az,
                                         double bx, double by, double bz, double (&j)[6], double &r)
{
    const double s = ((ax * bx + ay * by) + az * bz) < 0.0 ? -1.0 : 1.0;
    const double nx = 0.5 * (bx + s * ax), ny = 0.5 * (by + s * ay), nz = 0.5 * (bz + s * az);
    const double m0 = a0 + b0, m1 = a1 + b1, m2 = a2 + b2;
    r = (nx * (a0 - b0) + ny * (a1 - b1)) + nz * (a2 - b2);
    j[0] = m1 * nz - m2 * ny; j[1] = m2 * nx - m0 * nz; j[2] = m0 * ny - m1 * nx;
    j[3] = nx; j[4] = ny; j[5] = nz;
}

// a float32 source normal (slot i of src_n) -> unit fp64 in plane_normal's order, n * (1 / sqrt(n2)); false: zero or non-finite length
__device__ __forceinline__ bool symm_source_normal(const float *__restrict__ src_n, long long i, double &sx, double &sy, double &sz)
{
    const double s0 = (double)src_n[3 * i], s1 = (double)src_n[3 * i + 1], s2 = (double)src_n[3 * i + 2];
    const double n2 = (s0 * s0 + s1 * s1) + s2 * s2;
    if (!(n2 > 0.0) || !(n2 < INFINITY)) return false;
    const double inv = 1.0 / sqrt(n2);
    sx = s0 * inv; sy = s1 * inv; sz = s2 * inv;
    return true;
}

// a pair's contribution to the row, in three slices of 12 + 12 + 8 sums (NSUMS_PLANE's layout)
__device__ __forceinline__ void plane_terms_0(const double (&j)[6], double (&h)[12])
{
    h[0] = j[0] * j[0]; h[1] = j[0] * j[1]; h[2] = j[0] * j[2]; h[3] = j[0] * j[3]; h[4] = j[0] * j[4]; h[5] = j[0] * j[5];
    h[6] = j[1] * j[1]; h[7] = j[1] * j[2]; h[8] = j[1] * j[3]; h[9] = j[1] * j[4]; h[10] = j[1] * j[5]; h[11] = j[2] * j[2];
}
__device__ __forceinline__ void plane_terms_1(const double (&j)[6], double r, double (&h)[12])
{
    h[0] = j[2] * j[3]; h[1] = j[2] * j[4]; h[2] = j[2] * j[5]; h[3] = j[3] * j[3]; h[4] = j[3] * j[4]; h[5] = j[3] * j[5];
    h[6] = j[4] * j[4]; h[7] = j[4] * j[5]; h[8] = j[5] * j[5]; h[9] = j[0] * r; h[10] = j[1] * r; h[11] = j[2] * r;
}
__device__ __forceinline__ void plane_terms_2(const double (&j)[6], double r, double one, double dd, double (&h)[8])
{
    h[0] = j[3] * r; h[1] = j[4] * r; h[2] = j[5] * r; h[3] = one; h[4] = dd; h[5] = dd * dd; h[6] = r * r; h[7] = 0.0;
}

// the waves' rows in red -> the workgroup's row, waves in order.  Called by ALL threads, after the last slice.
__device__ __forceinline__ void block_finish_plane(double (*red)[NSUMS_PLANE], double *__restrict__ row)
{
    __syncthreads();
    if (threadIdx.x < NSUMS_PLANE) {
        double v = red[0][threadIdx.x];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) v += red[w][threadIdx.x];
        row[threadIdx.x] = v;
    }
}

// block_store_pair for the plane row: ONE pair per lane, formed and reduced slice by slice (the same reduce-scatter), so the
// epilogue never holds 32 sums and the butterfly's temporaries at once.  red: __shared__ double[blockDim.x / 64][NSUMS_PLANE].
// WEIGHTED: the pair's w multiplies its J J^T and J r terms and is itself summed into P_W; K, the distance sums and sum r^2 stay
// as they are.  The unweighted instance is the code it was.
template <bool WEIGHTED = false>
__device__ __forceinline__ void block_store_plane(bool valid, const double (&jj)[6], double r, double dd, double (*red)[NSUMS_PLANE],
                                                  double *__restrict__ row, double w = 0.0)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double j[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) j[k] = valid ? jj[k] : 0.0;
    if (!valid) { r = 0.0; dd = 0.0; }
    if constexpr (WEIGHTED) { if (!valid) w = 0.0; }
    {
        double h[12];
        plane_terms_0(j, h);
        if constexpr (WEIGHTED) {
#pragma unroll
            for (int k = 0; k < 12; ++k) h[k] *= w;
        }
        wave_reduce_scatter<12>(h, lane, &red[wave][0]);
    }
    {
        double h[12];
        plane_terms_1(j, r, h);
        if constexpr (WEIGHTED) {
#pragma unroll
            for (int k = 0; k < 12; ++k) h[k] *= w;
        }
        wave_reduce_scatter<12>(h, lane, &red[wave][12]);
    }
    {
        double h[8];
        plane_terms_2(j, r, valid ? 1.0 : 0.0, dd, h);
        if constexpr (WEIGHTED) { h[0] *= w; h[1] *= w; h[2] *= w; h[7] = w; }
        wave_reduce_scatter<8>(h, lane, &red[wave][24]);
    }
    block_finish_plane(red, row);
}

// k_pair_accumulate_canon for the plane metric: the same pair with the metric's normal (pair_fetch<true, true>), then the
// plane row.  One thread per source slot; plane_tn: vertex mode, one base-local normal per target
// vertex (surface mode: nullptr, the nearest triangle's geometric normal in the operand order of the normal-angle test).
// Its workgroups depend on the shard size alone, so every search mode leaves the same rows.
// WEIGHTED (oa_set_robust / oa_set_source_weights): w = w_vertex * psi(res_scale * |r|), r the plane residual the row is built
// from -- the distance to the tangent plane in world units, NOT the pair distance, which would down-weight exactly the sliding
// pairs this metric exists for; w_slot = one weight per slot (nullptr: all 1).  The unweighted instance never reads either.
constexpr int PLANE_THREADS = 512;
constexpr int PLANE_MAX_BLOCKS = 16384;
#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
template <bool WEIGHTED, bool RECIP = false>
__global__ __launch_bounds__(PLANE_THREADS) void k_pair_accumulate_plane(const DevState *__restrict__ st, const float4 *__restrict__ src4,
                                                               int ns, const float *__restrict__ tgt_xyz,
                                                               unsigned long long *__restrict__ keys, int *__restrict__ prev,
                                                               float4 *__restrict__ win, const float4 *__restrict__ tri9,
                                                               PairTest<RECIP> nrm, const float *__restrict__ plane_tn,
                                                               const float *__restrict__ w_slot, double *__restrict__ partials,
                                                               unsigned long long *__restrict__ t_acc_start)
{
    __shared__ double red[PLANE_THREADS / 64][NSUMS_PLANE];
    if (t_acc_start && blockIdx.x == 0 && threadIdx.x == 0) *t_acc_start = wall_clock64();   // ~ the end of the search
    if (st->halt) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = false;
    double nx = 0.0, ny = 0.0, nz = 0.0;
    PairFetch f = {};
    if (i < ns) {
        valid = pair_fetch<true, true, RECIP>(st, src4, i, tgt_xyz, keys, prev, win, tri9, nrm, plane_tn, st->thresh, f);
        if (valid) valid = plane_normal(st, f.tn, nx, ny, nz);
    }
    const double pvx = st->pivot[0], pvy = st->pivot[1], pvz = st->pivot[2];
    double j[6], r;
    plane_row((double)f.p.x - pvx, (double)f.p.y - pvy, (double)f.p.z - pvz, (double)f.bx - pvx, (double)f.by - pvy, (double)f.bz - pvz, nx, ny, nz, j, r);
    if constexpr (WEIGHTED) {
        double w = 0.0;
        if (valid) {
            w = robust_psi(st->loss, st->res_scale * fabs(r), st->robust_c);
            if (w_slot) w *= (double)w_slot[i];
        }
        block_store_plane<true>(valid, j, r, f.dist - st->d_pivot, red, partials + (long long)blockIdx.x * NSUMS_PLANE, w);
    } else
        block_store_plane(valid, j, r, f.dist - st->d_pivot, red, partials + (long long)blockIdx.x * NSUMS_PLANE);
}

// k_pair_accumulate_plane's sibling for the symmetric metric: the same pair_fetch<true, true> and plane_normal for n_b, the slot's
// source normal as k_pair_accumulate_gicp reads it (src_n: float32, align-local, slot order; zero or non-finite length drops the
// pair from the step and from K), symm_row in plane_row's place, then the same block_store_plane -- the plane row's layout, reduce
// and solve.  Launched like the plane kernel (plane_threads / plane_blocks).  WEIGHTED: w = w_vertex * psi(res_scale * |r|).
template <bool WEIGHTED, bool RECIP = false>
__global__ __launch_bounds__(PLANE_THREADS) void k_pair_accumulate_symm(const DevState *__restrict__ st, const float4 *__restrict__ src4,
                                                              int ns, const float *__restrict__ tgt_xyz,
                                                              unsigned long long *__restrict__ keys, int *__restrict__ prev,
                                                              float4 *__restrict__ win, const float4 *__restrict__ tri9,
                                                              PairTest<RECIP> nrm, const float *__restrict__ plane_tn,
                                                              const float *__restrict__ src_n, const float *__restrict__ w_slot,
                                                              double *__restrict__ partials, unsigned long long *__restrict__ t_acc_start)
{
    __shared__ double red[PLANE_THREADS / 64][NSUMS_PLANE];
    if (t_acc_start && blockIdx.x == 0 && threadIdx.x == 0) *t_acc_start = wall_clock64();   // ~ the end of the search
    if (st->halt) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = false;
    double nx = 0.0, ny = 0.0, nz = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
    PairFetch f = {};
    if (i < ns) {
        valid = pair_fetch<true, true, RECIP>(st, src4, i, tgt_xyz, keys, prev, win, tri9, nrm, plane_tn, st->thresh, f);
        if (valid) valid = plane_normal(st, f.tn, nx, ny, nz);
        if (valid) valid = symm_source_normal(src_n, i, sx, sy, sz);
    }
    const double pvx = st->pivot[0], pvy = st->pivot[1], pvz = st->pivot[2];
    double j[6], r;
    symm_row((double)f.p.x - pvx, (double)f.p.y - pvy, (double)f.p.z - pvz, (double)f.bx - pvx, (double)f.by - pvy, (double)f.bz - pvz,
             sx, sy, sz, nx, ny, nz, j, r);
    if constexpr (WEIGHTED) {
        double w = 0.0;
        if (valid) {
            w = robust_psi(st->loss, st->res_scale * fabs(r), st->robust_c);
            if (w_slot) w *= (double)w_slot[i];
        }
        block_store_plane<true>(valid, j, r, f.dist - st->d_pivot, red, partials + (long long)blockIdx.x * NSUMS_PLANE, w);
    } else
        block_store_plane(valid, j, r, f.dist - st->d_pivot, red, partials + (long long)blockIdx.x * NSUMS_PLANE);
}
#endif  // !OA_FAMILY_TU

// ---- the plane-to-plane metric (Generalized-ICP, Segal et al. 2009; oa_set_metric(OA_METRIC_GICP)) ---------------------------
// A pair is weighted by W = 2 eps M^-1, M = C_a + C_b = 2 I - (1 - eps)(n_a n_a^T + n_b n_b^T): the regularised covariances of
// the paper (eigenvalues 1, 1, eps, the eps-axis along the normal) of both sides, both in align-local space.  M is symmetric
// with eigenvalues in [2 eps, 2]: adjugate over determinant, ONE division.  The factor 2 eps does not move the step; with it
// e^T W e -> (n . e)^2 for n_a = n_b as eps -> 0, the plane metric's residual.  Only n n^T enters: the normals' signs drop out.
// na, nb unit.  W: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2).
__device__ __forceinline__ void gicp_weight(double eps, double ax, double ay, double az, double bx, double by, double bz, double (&W)[6])
{
    const double k = 1.0 - eps;
    const double m00 = 2.0 - k * (ax * ax + bx * bx), m01 = -k * (ax * ay + bx * by), m02 = -k * (ax * az + bx * bz);
    const double m11 = 2.0 - k * (ay * ay + by * by), m12 = -k * (ay * az + by * bz), m22 = 2.0 - k * (az * az + bz * bz);
    const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
    const double det = (m00 * c00 + m01 * c01) + m02 * c02;
    const double s = (2.0 * eps) / det;
    W[0] = s * c00; W[1] = s * c01; W[2] = s * c02; W[3] = s * c11; W[4] = s * c12; W[5] = s * c22;
}

// row i of C = [a]x W (the upper right block of J^T W J: column k of C is a x W_k)
__device__ __forceinline__ void gicp_c_row(int i, double a0, double a1, double a2, const double (&W)[6], double (&c)[3])
{
    if (i == 0)      { c[0] = a1 * W[2] - a2 * W[1]; c[1] = a1 * W[4] - a2 * W[3]; c[2] = a1 * W[5] - a2 * W[4]; }
    else if (i == 1) { c[0] = a2 * W[0] - a0 * W[2]; c[1] = a2 * W[1] - a0 * W[4]; c[2] = a2 * W[2] - a0 * W[5]; }
    else             { c[0] = a0 * W[1] - a1 * W[0]; c[1] = a0 * W[3] - a1 * W[1]; c[2] = a0 * W[4] - a1 * W[2]; }
}

// block_store_plane for this metric.  The row is not rank one, so the 21 + 6 terms are formed from a', W and u = W e inside
// each slice (the upper left block of J^T W J: row i is a x (row i of C)); what stays live across the slices is a', W, u and
// four scalars -- never 32 sums and the butterfly's temporaries at once.  rr = e^T W e; w: as in block_store_plane.
template <bool WEIGHTED>
__device__ __forceinline__ void block_store_gicp(bool valid, double a0, double a1, double a2, const double (&Wp)[6], double u0, double u1,
                                                 double u2, double rr, double dd, double (*red)[NSUMS_PLANE], double *__restrict__ row,
                                                 double w = 0.0)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double W[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) W[k] = valid ? Wp[k] : 0.0;
    if (!valid) { a0 = a1 = a2 = 0.0; u0 = u1 = u2 = 0.0; rr = 0.0; dd = 0.0; w = 0.0; }
    {
        double h[12], c0[3], c1[3], c2[3];
        gicp_c_row(0, a0, a1, a2, W, c0);
        gicp_c_row(1, a0, a1, a2, W, c1);
        gicp_c_row(2, a0, a1, a2, W, c2);
        h[0] = a1 * c0[2] - a2 * c0[1]; h[1] = a2 * c0[0] - a0 * c0[2]; h[2] = a0 * c0[1] - a1 * c0[0];      // (0,0) (0,1) (0,2)
        h[3] = c0[0]; h[4] = c0[1]; h[5] = c0[2];                                                            // (0,3) (0,4) (0,5)
        h[6] = a2 * c1[0] - a0 * c1[2]; h[7] = a0 * c1[1] - a1 * c1[0];                                      // (1,1) (1,2)
        h[8] = c1[0]; h[9] = c1[1]; h[10] = c1[2];                                                           // (1,3) (1,4) (1,5)
        h[11] = a0 * c2[1] - a1 * c2[0];                                                                     // (2,2)
        if constexpr (WEIGHTED) {
#pragma unroll
            for (int k = 0; k < 12; ++k) h[k] *= w;
        }
        wave_reduce_scatter<12>(h, lane, &red[wave][0]);
    }
    {
        double h[12], c2[3];
        gicp_c_row(2, a0, a1, a2, W, c2);
        h[0] = c2[0]; h[1] = c2[1]; h[2] = c2[2];                                                            // (2,3) (2,4) (2,5)
        h[3] = W[0]; h[4] = W[1]; h[5] = W[2]; h[6] = W[3]; h[7] = W[4]; h[8] = W[5];                        // (3,3) .. (5,5)
        h[9] = a1 * u2 - a2 * u1; h[10] = a2 * u0 - a0 * u2; h[11] = a0 * u1 - a1 * u0;                      // a' x u
        if constexpr (WEIGHTED) {
#pragma unroll
            for (int k = 0; k < 12; ++k) h[k] *= w;
        }
        wave_reduce_scatter<12>(h, lane, &red[wave][12]);
    }
    {
        double h[8] = { u0, u1, u2, valid ? 1.0 : 0.0, dd, dd * dd, rr, 0.0 };
        if constexpr (WEIGHTED) { h[0] *= w; h[1] *= w; h[2] *= w; h[7] = w; }
        wave_reduce_scatter<8>(h, lane, &red[wave][24]);
    }
    block_finish_plane(red, row);
}

// k_pair_accumulate_plane for this metric: the same pair_fetch<true, true> and plane_normal for n_b, plus the
// slot's source normal (src_n: float32, align-local, slot order; normalised in fp64 in plane_normal's order, n * (1 / sqrt(n2));
// zero or non-finite length drops the pair from the step and from K, as a zero n_b does).  Launched like the plane kernel
// (plane_threads / plane_blocks).  WEIGHTED: w = w_vertex * psi(res_scale * sqrt(e^T W e)).
#if !defined(OA_FAMILY_TU)
template <bool WEIGHTED, bool RECIP = false>
__global__ __launch_bounds__(PLANE_THREADS) void k_pair_accumulate_gicp(const DevState *__restrict__ st, const float4 *__restrict__ src4,
                                                              int ns, const float *__restrict__ tgt_xyz,
                                                              unsigned long long *__restrict__ keys, int *__restrict__ prev,
                                                              float4 *__restrict__ win, const float4 *__restrict__ tri9,
                                                              PairTest<RECIP> nrm, const float *__restrict__ plane_tn,
                                                              const float *__restrict__ src_n, const float *__restrict__ w_slot,
                                                              double *__restrict__ partials, unsigned long long *__restrict__ t_acc_start)
{
    __shared__ double red[PLANE_THREADS / 64][NSUMS_PLANE];
    if (t_acc_start && blockIdx.x == 0 && threadIdx.x == 0) *t_acc_start = wall_clock64();   // ~ the end of the search
    if (st->halt) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = false;
    double nx = 0.0, ny = 0.0, nz = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
    PairFetch f = {};
    if (i < ns) {
        valid = pair_fetch<true, true, RECIP>(st, src4, i, tgt_xyz, keys, prev, win, tri9, nrm, plane_tn, st->thresh, f);
        if (valid) valid = plane_normal(st, f.tn, nx, ny, nz);
        if (valid) {
            const double s0 = (double)src_n[3ll * i], s1 = (double)src_n[3ll * i + 1], s2 = (double)src_n[3ll * i + 2];
            const double n2 = (s0 * s0 + s1 * s1) + s2 * s2;
            valid = (n2 > 0.0) && (n2 < INFINITY);
            const double inv = 1.0 / sqrt(n2);
            sx = s0 * inv; sy = s1 * inv; sz = s2 * inv;
        }
    }
    const double pvx = st->pivot[0], pvy = st->pivot[1], pvz = st->pivot[2];
    const double a0 = (double)f.p.x - pvx, a1 = (double)f.p.y - pvy, a2 = (double)f.p.z - pvz;
    const double e0 = a0 - ((double)f.bx - pvx), e1 = a1 - ((double)f.by - pvy), e2 = a2 - ((double)f.bz - pvz);
    double W[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    if (valid) gicp_weight(st->gicp_eps, sx, sy, sz, nx, ny, nz, W);
    const double u0 = (W[0] * e0 + W[1] * e1) + W[2] * e2, u1 = (W[1] * e0 + W[3] * e1) + W[4] * e2, u2 = (W[2] * e0 + W[4] * e1) + W[5] * e2;
    const double rr = (e0 * u0 + e1 * u1) + e2 * u2;
    double w = 0.0;
    if constexpr (WEIGHTED) {
        if (valid) {
            w = robust_psi(st->loss, st->res_scale * sqrt(fmax(rr, 0.0)), st->robust_c);
            if (w_slot) w *= (double)w_slot[i];
        }
    }
    block_store_gicp<WEIGHTED>(valid, a0, a1, a2, W, u0, u1, u2, rr, f.dist - st->d_pivot, red, partials + (long long)blockIdx.x * NSUMS_PLANE, w);
}
#endif  // !OA_FAMILY_TU

// ---- the loss's scale from the step's own residuals (oa_set_robust_auto): an exact order statistic on the device --------
// c = max(m q, c_min), q the k-th smallest (k = ceil(p K_q), 1-based) of the K_q residuals of this step's pairs that are counted
// in K and carry a vertex weight > 0, each rounded to float32.  The bits of a non-negative float order as unsigned integers, so
// q is found by a radix select over its 32-bit key, most significant digit first, 11 + 11 + 10 bits: count the keys per digit
// (SEL_BINS bins: in LDS per workgroup, merged with integer atomicAdd -- any order gives the same counts), walk the counts to
// the bin that holds rank k, go on among the keys that share the digits found so far.  Per iteration, between the search and
// the weighted accumulation:
//   k_residual_keys   one thread per slot: the pair k_pair_accumulate_weighted / _plane<true> is about to form, read-only
//                     (keys, prev, win stay as the search left them) -> its key (RKEY_NONE: takes no part) + level 0's counts
//   k_select_scan 0   one workgroup: K_q, k, level 0's bin
//   k_select_hist 1, k_select_scan 1, k_select_hist 2     over the 4-byte keys only
//   k_select_scan 2   q, robust_c = max(m q, c_min) into DevState (what the accumulation reads), the three histograms zeroed
// i.e. six short launches, no host round trip, no float atomics: the same bits whatever order the workgroups run in.
constexpr uint32_t RKEY_NONE = 0xFFFFFFFFu;
constexpr int SEL_BINS = 2048, SEL_LEVELS = 3;
constexpr int SEL_THREADS = 256;          // k_select_hist, k_select_scan
constexpr int SEL_HIST_MAX_BLOCKS = 1024; // k_select_hist strides over the keys
__host__ __device__ inline uint32_t sel_digit(uint32_t key, int level)
{
    return level == 0 ? key >> 21 : level == 1 ? (key >> 10) & 2047u : key & 1023u;
}
// the digits above `level`'s: what sel_prefix holds when that level is counted
__host__ __device__ inline uint32_t sel_above(uint32_t key, int level) { return level == 1 ? key >> 21 : key >> 10; }

// (sel_count / sel_clear / sel_flush are inlined helpers: the family units see them too -- oa_trim.hpp's GICP keys kernel)
// one key into the workgroup's LDS counts.  The residuals of a step share their exponent, so the lanes of a wave hit a
// handful of bins at level 0 and same-address LDS atomics take turns: up to four rounds in which the first pending lane's bin
// is counted for every lane that shares it by ONE add, and whatever is left adds for itself.  Called by ALL lanes of the wave.
__device__ __forceinline__ void sel_count(uint32_t *bins, bool active, uint32_t b)
{
    const int lane = threadIdx.x & 63;
    for (int round = 0; round < 4; ++round) {
        const unsigned long long pending = __ballot(active);
        if (!pending) break;                                        // (wave-uniform)
        const int leader = __ffsll((long long)pending) - 1;
        const uint32_t lb = (uint32_t)__shfl((int)b, leader, 64);
        const bool mine = active && b == lb;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(&bins[lb], (uint32_t)__popcll(same));
        if (mine) active = false;
    }
    if (active) atomicAdd(&bins[b], 1u);
}
__device__ __forceinline__ void sel_clear(uint32_t *bins)
{
    for (int b = threadIdx.x; b < SEL_BINS; b += blockDim.x) bins[b] = 0u;
    __syncthreads();
}
__device__ __forceinline__ void sel_flush(const uint32_t *bins, uint32_t *__restrict__ hist)
{
    __syncthreads();
    for (int b = threadIdx.x; b < SEL_BINS; b += blockDim.x) {
        const uint32_t v = bins[b];
        if (v) atomicAdd(&hist[b], v);
    }
}

#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
// The residual of every slot's pair, as the weighted accumulation of this metric will see it: pair_fetch<false, PLANE> (the same
// pair, NO write to keys, prev or win) and -- PLANE -- plane_normal / plane_row.  rkeys[i] = the bits of (float)residual (point: pair_eval's dist; plane: res_scale |n . (a' - b')|), or
// RKEY_NONE for a slot without a pair counted in K or with vertex weight 0.  Launched like the accumulation (plane_threads /
// plane_blocks); stamps the end of the search in its place.
template <bool PLANE, bool RECIP = false>
__global__ __launch_bounds__(PLANE_THREADS) void k_residual_keys(const DevState *__restrict__ st, const float4 *__restrict__ src4, int ns,
                                                             const float *__restrict__ tgt_xyz,
                                                             const unsigned long long *__restrict__ keys,
                                                             const float4 *__restrict__ win, const float4 *__restrict__ tri9,
                                                             PairTest<RECIP> nrm, const float *__restrict__ plane_tn,
                                                             const float *__restrict__ w_slot, uint32_t *__restrict__ rkeys,
                                                             uint32_t *__restrict__ hist, unsigned long long *__restrict__ t_acc_start)
{
    __shared__ uint32_t bins[SEL_BINS];
    if (t_acc_start && blockIdx.x == 0 && threadIdx.x == 0) *t_acc_start = wall_clock64();   // ~ the end of the search
    if (st->halt) return;
    sel_clear(bins);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t rkey = RKEY_NONE;
    if (i < ns) {
        PairFetch f;
        if (pair_fetch<false, PLANE, RECIP>(st, src4, i, tgt_xyz, keys, nullptr, win, tri9, nrm, plane_tn, st->thresh, f)) {
            bool valid = true;
            double res = f.dist;
            if constexpr (PLANE) {
                double nx = 0.0, ny = 0.0, nz = 0.0;
                valid = plane_normal(st, f.tn, nx, ny, nz);
                const double pvx = st->pivot[0], pvy = st->pivot[1], pvz = st->pivot[2];
                double j[6], r;
                plane_row((double)f.p.x - pvx, (double)f.p.y - pvy, (double)f.p.z - pvz, (double)f.bx - pvx, (double)f.by - pvy, (double)f.bz - pvz,
                          nx, ny, nz, j, r);
                res = st->res_scale * fabs(r);
            }
            if (valid && w_slot) valid = w_slot[i] > 0.f;
            if (valid) rkey = (uint32_t)__float_as_int((float)res);
        }
        rkeys[i] = rkey;
    }
    sel_count(bins, rkey != RKEY_NONE, sel_digit(rkey, 0));
    sel_flush(bins, hist);
}

// levels 1 and 2: the counts of this level's digit among the keys whose higher digits are the ones found so far
__global__ __launch_bounds__(SEL_THREADS) void k_select_hist(const DevState *__restrict__ st, const uint32_t *__restrict__ rkeys, int ns,
                                                          int level, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t bins[SEL_BINS];
    if (st->halt || st->robust_kq == 0u) return;
    sel_clear(bins);
    const uint32_t prefix = st->sel_prefix;
    // (whole waves leave the loop together: sel_count is a wave's business)
    for (long long base = (long long)blockIdx.x * blockDim.x; base < ns; base += (long long)gridDim.x * blockDim.x) {
        const long long i = base + threadIdx.x;
        const uint32_t key = i < ns ? rkeys[i] : RKEY_NONE;
        sel_count(bins, key != RKEY_NONE && sel_above(key, level) == prefix, sel_digit(key, level));
    }
    sel_flush(bins, hist + (long long)level * SEL_BINS);
}

// one workgroup: walk `level`'s counts to the bin that holds the wanted rank.  Level 0 first takes K_q (all its counts) and the
// rank k - 1 = ceil(p K_q) - 1 from it; level 2 ends the selection: q, robust_c, the histograms back to zero.
__global__ __launch_bounds__(SEL_THREADS) void k_select_scan(DevState *__restrict__ st, uint32_t *__restrict__ hist, int level)
{
    constexpr int PER = SEL_BINS / SEL_THREADS;                     // consecutive bins per thread
    __shared__ uint32_t wave_tot[SEL_THREADS / 64];
    if (st->halt) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t *h = hist + (long long)level * SEL_BINS;
    uint32_t cnt[PER], mine = 0u;
#pragma unroll
    for (int k = 0; k < PER; ++k) { cnt[k] = h[threadIdx.x * PER + k]; mine += cnt[k]; }
    uint32_t incl = mine;                                           // inclusive scan over the wave, then the waves in order
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine, total = 0u;
    for (int w = 0; w < SEL_THREADS / 64; ++w) { if (w < wave) before += wave_tot[w]; total += wave_tot[w]; }
    uint32_t rank = st->sel_rank, prefix = st->sel_prefix, kq = st->robust_kq;
    if (level == 0) {
        kq = total;
        prefix = 0u;
        double k = ceil(st->robust_p * (double)kq);
        k = k < 1.0 ? 1.0 : (k > (double)kq ? (double)kq : k);
        rank = (uint32_t)k - 1u;
    }
    __syncthreads();                                                // (every thread has read DevState before one of them writes it)
    if (kq != 0u && rank >= before && rank - before < mine) {       // exactly one thread
        uint32_t r = rank - before, bin = threadIdx.x * PER;
        bool found = false;
#pragma unroll
        for (int k = 0; k < PER; ++k) {                             // (unrolled: cnt stays in registers)
            if (!found && r < cnt[k]) found = true;
            if (!found) { r -= cnt[k]; ++bin; }
        }
        prefix = level == 2 ? (prefix << 10) | bin : (prefix << 11) | bin;
        st->sel_prefix = prefix;
        st->sel_rank = r;
        if (level == 0) st->robust_kq = kq;
        if (level == SEL_LEVELS - 1) {
            const double q = (double)__uint_as_float(prefix);
            const double c = st->robust_mult * q;
            st->robust_q = q;
            st->robust_c = c > st->robust_cmin ? c : st->robust_cmin;
        }
    }
    if (kq == 0u && threadIdx.x == 0 && level == 0) {               // nothing took part: the floor (the later launches return at once)
        st->robust_kq = 0u; st->sel_prefix = 0u; st->sel_rank = 0u;
        st->robust_q = 0.0;
        st->robust_c = st->robust_cmin;
    }
    if (level == SEL_LEVELS - 1 || kq == 0u)
        for (int b = threadIdx.x; b < SEL_LEVELS * SEL_BINS; b += SEL_THREADS) hist[b] = 0u;
}
#endif  // !OA_FAMILY_TU

// ---- fixed-order reduction of the rows of per-workgroup partials (bitwise reproducible, no float atomics) -------------
// A row is NSUMS doubles = 12 x 16 bytes.  1024 threads = 85 slices of 12 threads: slice s adds rows s, s + 85, ... in
// order (thread c of a slice owns columns 2c, 2c + 1 and loads them as one 16-byte word, 16 rows in flight per thread),
// then the slices are added in order.  Round 2's version (32 slices of 32 threads, 8 rows in flight) was sized for the
// <= 512 rows of k_pair_accumulate; the search kernels that accumulate in their epilogue write one row per workgroup,
// up to 4096 of them, and a chain of 16 round trips per thread would cost more than the launch the fusion saves.
constexpr int RED_THREADS = 1024;

// rows [0, n_rows) of `rows` -> out[0 .. W) (shared or global).  Called by all RED_THREADS threads of a workgroup.
// W = doubles per row: NSUMS (the numbers above) or NSUMS_PLANE (16 threads per row, 64 slices; same scheme).
template <int W = NSUMS>
__device__ __forceinline__ void reduce_rows_block(const double *__restrict__ rows, int n_rows, double *out)
{
    static_assert(W % 2 == 0 && W <= 64, "a thread owns two columns of a row");
    constexpr int TPR = W / 2;                          // threads per row: 12
    constexpr int RED_SLICES = RED_THREADS / TPR;       // 85
    __shared__ double red[RED_SLICES][W];
    const int s = threadIdx.x / TPR, c = threadIdx.x - TPR * s;
    if (s < RED_SLICES) {
        double v0 = 0.0, v1 = 0.0;
        const double2 *__restrict__ col = (const double2 *)rows + c;       // row r, columns 2c, 2c+1: col[TPR r]
        int r = s;
        for (; r + 15 * RED_SLICES < n_rows; r += 16 * RED_SLICES) {
            double2 p[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) p[u] = col[(long long)TPR * (r + RED_SLICES * u)];
#pragma unroll
            for (int u = 0; u < 16; ++u) { v0 += p[u].x; v1 += p[u].y; }
        }
        // the last (or only) batch, fewer than 16 rows: all loads at once, predicated -- ONE round trip where batches of four and
        // single rows took up to five (1954 rows at 1M points: 23 per slice = 16 + 4 + 1 + 1 + 1); same additions, same order.
        // (Four wide when that covers it: a few hundred rows are a 2562-point problem, where every instruction shows.)
        if (r + 4 * RED_SLICES < n_rows) {
            double2 p[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int rr = r + RED_SLICES * u;
                p[u] = make_double2(0.0, 0.0);
                if (rr < n_rows) p[u] = col[(long long)TPR * rr];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (r + RED_SLICES * u < n_rows) { v0 += p[u].x; v1 += p[u].y; }
        } else if (r < n_rows) {
            double2 p[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int rr = r + RED_SLICES * u;
                p[u] = make_double2(0.0, 0.0);
                if (rr < n_rows) p[u] = col[(long long)TPR * rr];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (r + RED_SLICES * u < n_rows) { v0 += p[u].x; v1 += p[u].y; }
        }
        red[s][2 * c] = v0; red[s][2 * c + 1] = v1;
    }
    __syncthreads();
    if (threadIdx.x < W) {
        double t = red[0][threadIdx.x];
        for (int k = 1; k < RED_SLICES; ++k) t += red[k][threadIdx.x];
        out[threadIdx.x] = t;
    }
}

// How many rows a reduce launch has to add up.  Shards in the zone where the tree and the grid search take turns
// (DevState::tree_turn) have both searches enqueued and only one of them writes rows: the count is picked on the device.
struct RowSel {
    int n, n_tree;      // rows (of the grid search / the only search); rows the whole-tree search writes
    int by_turn;        // 1: n_tree when DevState::tree_turn, n otherwise
};
__device__ __forceinline__ int rows_of(const RowSel &sel, const DevState *st)
{
    return (sel.by_turn && st->tree_turn != 0) ? sel.n_tree : sel.n;
}

// stamp: where the launch leaves wall_clock64() at its start (the end of the search + accumulate part of the iteration,
// DevState::t_acc_start), or nullptr
#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
__global__ __launch_bounds__(RED_THREADS) void k_reduce_partials(const DevState *__restrict__ st, const double *__restrict__ partials,
                                                                 RowSel sel, double *__restrict__ sums_out,
                                                                 unsigned long long *__restrict__ stamp)
{
    if (stamp && threadIdx.x == 0) *stamp = wall_clock64();
    reduce_rows_block(partials, st ? rows_of(sel, st) : sel.n, sums_out);
    // what follows this launch in the stream is the exchange of the sums (ncclAllReduce): the host's watchdog times THAT wait --
    // "entered the collective of iteration n + 1" here, "iteration n + 1 done" (host_halt[1]) from the solve behind it -- not
    // the search in front of it, which may take longer than any time limit without anything being wrong
    if (st && st->host_halt && threadIdx.x == 0) st->host_halt[5] = st->n + 1;
    if (st && threadIdx.x == 0) const_cast<DevState *>(st)->t_xchg_start = wall_clock64();
}

// sums over explicit pairs (contract 2: oa_kabsch).  A, B: 3 x K row-major with leading dimension ld.
__global__ __launch_bounds__(ACC_THREADS) void k_accumulate_pairs(const double *__restrict__ A,
                                                                  const double *__restrict__ B, long long K,
                                                                  long long ld, double pvx, double pvy, double pvz,
                                                                  double *__restrict__ partials)
{
    __shared__ double red[ACC_THREADS / 64][NSUMS];
    double acc[NSUMS];
#pragma unroll
    for (int k = 0; k < NSUMS; ++k) acc[k] = 0.0;
    for (long long i = (long long)blockIdx.x * ACC_THREADS + threadIdx.x; i < K; i += (long long)gridDim.x * ACC_THREADS) {
        const double a0 = A[i] - pvx, a1 = A[ld + i] - pvy, a2 = A[2 * ld + i] - pvz;
        const double b0 = B[i] - pvx, b1 = B[ld + i] - pvy, b2 = B[2 * ld + i] - pvz;
        acc[S_A] += a0; acc[S_A + 1] += a1; acc[S_A + 2] += a2;
        acc[S_B] += b0; acc[S_B + 1] += b1; acc[S_B + 2] += b2;
        acc[S_H + 0] += b0 * a0; acc[S_H + 1] += b0 * a1; acc[S_H + 2] += b0 * a2;
        acc[S_H + 3] += b1 * a0; acc[S_H + 4] += b1 * a1; acc[S_H + 5] += b1 * a2;
        acc[S_H + 6] += b2 * a0; acc[S_H + 7] += b2 * a1; acc[S_H + 8] += b2 * a2;
        acc[S_AA] += (a0 * a0 + a1 * a1) + a2 * a2;
        acc[S_BB] += (b0 * b0 + b1 * b1) + b2 * b2;
        acc[S_K] += 1.0;
    }
    block_store_partial(acc, red, partials + (long long)blockIdx.x * NSUMS);
}

// one thread: solve only (oa_kabsch / oa_kabsch_from_sums).  out[0..15] = M, out[16] = ok flag
__global__ void k_solve_only(const double *__restrict__ sums, double pvx, double pvy, double pvz, int with_scale,
                             double *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s[NSUMS], M[16];
    for (int k = 0; k < NSUMS; ++k) s[k] = sums[k];
    const double pv[3] = { pvx, pvy, pvz };
    const bool ok = solve_from_sums(s, pv, (with_scale & 1) != 0, M, nullptr, false, (with_scale & 2) != 0);   // bit 1: Horn's quaternion branch
    for (int k = 0; k < 16; ++k) out[k] = ok ? M[k] : 0.0;
    out[16] = ok ? 1.0 : 0.0;
}

// the plane row over explicit pairs (oa_point_to_plane).  A, B, N: 3 x K row-major with leading dimension ld; N need not be unit
// (a pair whose normal has zero or non-finite length is left out, as in the loop).  No distances: sums P_D, P_DD stay 0.
__global__ __launch_bounds__(ACC_THREADS) void k_accumulate_pairs_plane(const double *__restrict__ A, const double *__restrict__ B,
                                                                        const double *__restrict__ N, long long K, long long ld,
                                                                        double pvx, double pvy, double pvz, double *__restrict__ partials)
{
    __shared__ double red[ACC_THREADS / 64][NSUMS_PLANE];
    double acc0[12], acc1[12], acc2[8];
#pragma unroll
    for (int k = 0; k < 12; ++k) { acc0[k] = 0.0; acc1[k] = 0.0; }
#pragma unroll
    for (int k = 0; k < 8; ++k) acc2[k] = 0.0;
    for (long long i = (long long)blockIdx.x * ACC_THREADS + threadIdx.x; i < K; i += (long long)gridDim.x * ACC_THREADS) {
        const double l0 = N[i], l1 = N[ld + i], l2 = N[2 * ld + i];
        const double n2 = (l0 * l0 + l1 * l1) + l2 * l2;
        if (!(n2 > 0.0) || !(n2 < INFINITY)) continue;
        const double inv = 1.0 / sqrt(n2);
        double j[6], r, h0[12], h1[12], h2[8];
        plane_row(A[i] - pvx, A[ld + i] - pvy, A[2 * ld + i] - pvz, B[i] - pvx, B[ld + i] - pvy, B[2 * ld + i] - pvz, l0 * inv, l1 * inv, l2 * inv, j, r);
        plane_terms_0(j, h0); plane_terms_1(j, r, h1); plane_terms_2(j, r, 1.0, 0.0, h2);
#pragma unroll
        for (int k = 0; k < 12; ++k) { acc0[k] += h0[k]; acc1[k] += h1[k]; }
#pragma unroll
        for (int k = 0; k < 8; ++k) acc2[k] += h2[k];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wave_reduce_scatter<12>(acc0, lane, &red[wave][0]);
    wave_reduce_scatter<12>(acc1, lane, &red[wave][12]);
    wave_reduce_scatter<8>(acc2, lane, &red[wave][24]);
    block_finish_plane(red, partials + (long long)blockIdx.x * NSUMS_PLANE);
}

// the symmetric row over explicit pairs (oa_symmetric_step): k_accumulate_pairs_plane with both sides' normals.  NA, NB need not
// be unit; a pair with a normal of zero or non-finite length on either side is left out.
__global__ __launch_bounds__(ACC_THREADS) void k_accumulate_pairs_symm(const double *__restrict__ A, const double *__restrict__ B,
                                                                       const double *__restrict__ NA, const double *__restrict__ NB,
                                                                       long long K, long long ld, double pvx, double pvy, double pvz,
                                                                       double *__restrict__ partials)
{
    __shared__ double red[ACC_THREADS / 64][NSUMS_PLANE];
    double acc0[12], acc1[12], acc2[8];
#pragma unroll
    for (int k = 0; k < 12; ++k) { acc0[k] = 0.0; acc1[k] = 0.0; }
#pragma unroll
    for (int k = 0; k < 8; ++k) acc2[k] = 0.0;
    for (long long i = (long long)blockIdx.x * ACC_THREADS + threadIdx.x; i < K; i += (long long)gridDim.x * ACC_THREADS) {
        const double p0 = NA[i], p1 = NA[ld + i], p2 = NA[2 * ld + i], q0 = NB[i], q1 = NB[ld + i], q2 = NB[2 * ld + i];
        const double pp = (p0 * p0 + p1 * p1) + p2 * p2, qq = (q0 * q0 + q1 * q1) + q2 * q2;
        if (!(pp > 0.0) || !(pp < INFINITY) || !(qq > 0.0) || !(qq < INFINITY)) continue;
        const double pinv = 1.0 / sqrt(pp), qinv = 1.0 / sqrt(qq);
        double j[6], r, h0[12], h1[12], h2[8];
        symm_row(A[i] - pvx, A[ld + i] - pvy, A[2 * ld + i] - pvz, B[i] - pvx, B[ld + i] - pvy, B[2 * ld + i] - pvz,
                 p0 * pinv, p1 * pinv, p2 * pinv, q0 * qinv, q1 * qinv, q2 * qinv, j, r);
        plane_terms_0(j, h0); plane_terms_1(j, r, h1); plane_terms_2(j, r, 1.0, 0.0, h2);
#pragma unroll
        for (int k = 0; k < 12; ++k) { acc0[k] += h0[k]; acc1[k] += h1[k]; }
#pragma unroll
        for (int k = 0; k < 8; ++k) acc2[k] += h2[k];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wave_reduce_scatter<12>(acc0, lane, &red[wave][0]);
    wave_reduce_scatter<12>(acc1, lane, &red[wave][12]);
    wave_reduce_scatter<8>(acc2, lane, &red[wave][24]);
    block_finish_plane(red, partials + (long long)blockIdx.x * NSUMS_PLANE);
}

// rows of the plane layout -> sums (oa_point_to_plane; the loop reduces inside k_reduce_solve_update_plane)
__global__ __launch_bounds__(RED_THREADS) void k_reduce_partials_plane(const double *__restrict__ partials, int n_rows, double *__restrict__ sums_out)
{
    reduce_rows_block<NSUMS_PLANE>(partials, n_rows, sums_out);
}

// one wave: the plane solve only (oa_point_to_plane; symmetric: oa_symmetric_step).  out[0..15] = M, out[16] = ok flag, out[17] = rank
__global__ __launch_bounds__(64) void k_solve_only_plane(const double *__restrict__ sums, double pvx, double pvy, double pvz, int symmetric,
                                                         double *__restrict__ out)
{
    __shared__ double sh_s[NSUMS_PLANE], sh_A[36], sh_V[36];
    const int lane = threadIdx.x;
    if (lane < NSUMS_PLANE) sh_s[lane] = sums[lane];
    __syncthreads();
    const double pv[3] = { pvx, pvy, pvz };
    double M[16];
    int rank;
    const bool ok = plane_solve_from_sums(sh_s, pv, sh_A, sh_V, lane < 6 ? lane : 6, lane < 6 ? lane + 1 : 6, M, rank, false, symmetric != 0);
    if (lane == 0) {
        for (int k = 0; k < 16; ++k) out[k] = ok ? M[k] : 0.0;
        out[16] = ok ? 1.0 : 0.0;
        out[17] = (double)rank;
    }
}
#endif  // !OA_FAMILY_TU

// ------------------------------------------------------------------------------------------------
// k_solve_update : operators/icp_align.py:106-149 (solve_update_block: two waves)
// ------------------------------------------------------------------------------------------------
// element `lane` (0..15) of m4_inverted(Af): the same sub-determinants, the same numerators, the same IEEE division as
// m4_inverted -- hence the same float -- but ONE division per lane instead of sixteen on one lane (they were a third of the
// post-solve chain).  Called by (at least) 16 lanes with the same Af; false if singular.
__device__ __forceinline__ bool m4_inverted_lane(const float *Af, int lane, float &out)
{
    float R[16], det;
    m4_adjoint_det(Af, R, det);
    if (det == 0.0f) return false;
    // element `lane` = (row j, column i) of the inverse = R[i][j] / det: a select chain instead of a dynamic index (registers)
    const int src = (lane & 3) * 4 + (lane >> 2);
    float nk = R[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) nk = (src == k) ? R[k] : nk;
    out = nk / det;
    return true;
}

// What follows the sums of an iteration (operators/icp_align.py:106-149), by a WORKGROUP of at least two waves; `sums`
// readable by all of them.  Called by ALL threads of the workgroup (it contains workgroup barriers); waves 2.. only pass.
//   wave 0, every lane redundantly (one lane's latency): the Kabsch solve (Jacobi, warm-started)           -> M, new_mat
//   then wave 0: matrix_world @ new_mat (lane k = element k), its inverse (lane k = element k: one division per lane),
//                |translation|, the convergence ring, n, halt, the report for the host
//        wave 1, at the same time: rotation angle (acos), d_stats (sqrt), the step record (lane k = element k of M and
//                new_mat), the angle ring, whose turn the next search is, d_pivot
// Round 2 ran all of it on one lane, one after the other: the part after the solve -- 64 products accumulated in double,
// 16 divisions, an acos, 40 stores -- took as long as the solve.
// snapshot of the loop state in LDS: every kernel that ends in solve_update_block takes it with one coalesced copy at its
// very start (the row reduction, or the wait for the mailboxes, runs meanwhile), so that the solve's reads of the state --
// three dependent global round trips on its critical path before -- are LDS reads.  Called by ALL threads; the caller's next
// __syncthreads() makes it visible.
__device__ __forceinline__ void snapshot_state(const DevState *__restrict__ st, DevState *sh)
{
    static_assert(sizeof(DevState) % 4 == 0, "DevState is copied word by word");
    for (int t = threadIdx.x; t < (int)(sizeof(DevState) / 4); t += blockDim.x) ((uint32_t *)sh)[t] = ((const uint32_t *)st)[t];
}

// PLANE: `sums` is a row of NSUMS_PLANE and the solve is plane_solve_from_sums (all of wave 0 together, its 6 x 6 in LDS); what
// follows M is the same code for both metrics.
template <bool PLANE = false>
__device__ __forceinline__ void solve_update_block(DevState *__restrict__ st, const DevState *cs, const double *sums,
                                                   StepRecord *__restrict__ hist, int *__restrict__ todo_count,
                                                   unsigned long long t_sums_in_hand = 0ull)
{
    constexpr int I_K = PLANE ? P_K : S_K, I_D = PLANE ? P_D : S_D, I_DD = PLANE ? P_DD : S_DD, I_W = PLANE ? P_W : S_W;
    // st: the loop state in global memory (written); cs: its snapshot from the start of this launch (read)
    __shared__ double sh_M[16];
    __shared__ float sh_new[16], sh_mw[16];
    __shared__ int sh_go;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x == 0) {
        // the grid search's hand-over list restarts empty; what it held -- entries, and the most any one wave handed over --
        // goes to the host, which decides from it whether the next grid search can finish its leftovers itself
        const int todo_n = todo_count ? todo_count[0] : 0, todo_wave_max = todo_count ? todo_count[1] : 0;
        if (todo_count) { todo_count[0] = 0; todo_count[1] = 0; }
        if (cs->host_halt) { cs->host_halt[2] = todo_n; cs->host_halt[3] = todo_wave_max; }
        sh_go = cs->halt ? 0 : 1;
    }
    __syncthreads();
    if (!sh_go) return;                                             // (uniform)
    if (wave == 0) {
        double M[16];
        double jv[9];
        bool ok;
        if constexpr (PLANE) {
            __shared__ double sh_A[36], sh_V[36];
            int rank;
            ok = plane_solve_from_sums(sums, cs->pivot, sh_A, sh_V, lane < 6 ? lane : 6, lane < 6 ? lane + 1 : 6, M, rank, cs->weighted != 0,
                                       cs->symmetric != 0);
            if (lane == 0) st->plane_rank = rank;
        } else {
            double s[NSUMS];
            for (int k = 0; k < NSUMS; ++k) s[k] = sums[k];
            const bool jv_valid = cs->jac_valid != 0;
            for (int k = 0; k < 9; ++k) jv[k] = jv_valid ? cs->jac_v[k] : 0.0;
            ok = solve_from_sums(s, cs->pivot, cs->with_scale != 0, M, jv, jv_valid, false, cs->weighted != 0);
        }
        if (lane == 0) {
            if (!ok) {                                              // K < 3 -> ValueError in the reference: OA_E_TOO_FEW_PAIRS
                st->status = -3; st->halt = 1; sh_go = 0;
                if (cs->host_halt) cs->host_halt[0] = 1;            // the enqueuing host stops here too (it would wait for progress that never comes)
            }
            else {
                if constexpr (!PLANE) {
                    for (int k = 0; k < 9; ++k) st->jac_v[k] = jv[k];
                    st->jac_valid = 1;
                }
                for (int k = 0; k < 16; ++k) { sh_M[k] = M[k]; sh_new[k] = (float)M[k]; }   // new_mat[y][z] = M[y][z]  (:116-119)
            }
        }
    }
    __syncthreads();
    if (!sh_go) return;
    const int n = cs->n;
    if (wave == 0) {
        // matrix_world @ new_mat (:121): element `lane`, the operation order of m4_mul_m4
        if (lane < 16) {
            const int i = lane >> 2, j = lane & 3;
            double acc = 0.0;
            for (int k = 0; k < 4; ++k) { const float p = cs->mx1[4 * i + k] * sh_new[4 * k + j]; acc += (double)p; }
            sh_mw[lane] = (float)acc;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // this wave's LDS writes above, its LDS reads below
        float mw[16];
        for (int k = 0; k < 16; ++k) mw[k] = sh_mw[k];
        if (lane < 16) st->mx1[lane] = mw[lane & 15];
        float inv_k = 0.f;
        const bool nonsingular = m4_inverted_lane(mw, lane & 15, inv_k);
        if (nonsingular && lane < 16) st->imx1[lane] = inv_k;
        if (lane == 0) {
            bool halt = false;
            if (!nonsingular) { st->status = -4; halt = true; }     // next make_pairs would raise   (general.py:265)
            const double trans = v3_length(sh_new[3], sh_new[7], sh_new[11]);   // new_mat.to_translation().length (:129,:138)
            bool converged = cs->converged != 0;
            if (cs->use_target) {                                   // if d_stats:                  (:136)
                st->ring_t[n % 5] = trans;                          // conv_t_list[i] = trans.length (:137-138)
                bool all = true;
                for (int k = 0; k < 5; ++k) all = all && ((k == n % 5 ? trans : cs->ring_t[k]) < cs->target_d);   // (:141)
                if (all) { converged = true; st->converged = 1; }
            }
            st->n = n + 1;                                          // n += 1                        (:151)
            if ((converged && cs->early_exit) || n + 1 >= cs->iters) halt = true;
            if (halt) st->halt = 1;
            st->t_prev_end = wall_clock64();                        // the next search starts (about) now
            if (cs->host_halt) {                                    // progress and halt flag for the enqueuing host
                // (no fence: the host only ever looks at these two words to decide whether to enqueue more; whichever arrives
                //  first, it enqueues an iteration too many -- which returns at once -- or stops where it should.  A system-scope
                //  fence here sat at the very end of every iteration's critical path.)
                cs->host_halt[1] = n + 1;
                if (halt) cs->host_halt[0] = 1;
            }
        }
    } else if (wave == 1) {
        double M[16];
        for (int k = 0; k < 16; ++k) M[k] = sh_M[k];
        const double trans = v3_length(sh_new[3], sh_new[7], sh_new[11]);
        const double angle = rotation_angle_3x3(M);
        const double K = sums[I_K];
        const double mean_dd = sums[I_D] / K;                       // mean of (d - d_pivot)
        const double mean_d = mean_dd + cs->d_pivot;
        double var = sums[I_DD] / K - mean_dd * mean_dd;
        if (var < 0.0) var = 0.0;
        if (hist && cs->max_records > 0) {
            StepRecord &r = hist[n % cs->max_records];
            if (lane < 16) { r.M[lane] = sh_M[lane]; r.new_mat[lane] = sh_new[lane]; }
            if (lane == 0) {
                r.K = K; r.mean_d = mean_d; r.std_d = sqrt(var); r.trans = trans; r.angle = angle;
                r.search_ticks = (cs->t_acc_start > cs->t_prev_end) ? (double)(cs->t_acc_start - cs->t_prev_end) : 0.0;
                r.exchange_ticks = (t_sums_in_hand > cs->t_xchg_start && cs->t_xchg_start) ? (double)(t_sums_in_hand - cs->t_xchg_start) : 0.0;
            }
        }
        if (lane == 0) {
            if (cs->use_target) st->ring_r[n % 5] = angle;
            st->d_pivot = mean_d;                                   // next iteration sums d relative to this mean
            st->weight_sum = cs->weighted ? sums[I_W] : K;
            // whose turn is the next search (DevState::tree_turn)
            const double moved = cs->use_target ? (trans + angle * cs->turn_scale) * cs->local_per_world : 0.0;
            st->tree_turn = (moved > cs->turn_limit) ? 1 : 0;
        }
    }
}

// loop start: the first search begins (about) now
#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
__global__ void k_stamp_start(DevState *__restrict__ st)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) st->t_prev_end = wall_clock64();
}

// split-phase form (one process per GPU): the sums come back from the all-reduce
__global__ __launch_bounds__(128) void k_solve_update(DevState *__restrict__ st, const double *__restrict__ sums, StepRecord *__restrict__ hist,
                               int *__restrict__ todo_count)
{
    __shared__ DevState cs;
    const unsigned long long t_in_hand = wall_clock64();            // behind the all-reduce in the stream: the world's sums are here
    snapshot_state(st, &cs);
    __syncthreads();
    solve_update_block(st, &cs, sums, hist, todo_count, t_in_hand);
}

// single-GPU form: the fixed-order reduction and the solve in one launch (same arithmetic, one boundary less)
__global__ __launch_bounds__(RED_THREADS) void k_reduce_solve_update(DevState *__restrict__ st, const double *__restrict__ partials,
                                                                     RowSel sel, double *__restrict__ sums_out,
                                                                     StepRecord *__restrict__ hist, int *__restrict__ todo_count, int stamp)
{
    __shared__ double sums[NSUMS];
    __shared__ DevState cs;
    const unsigned long long t_start = wall_clock64();
    snapshot_state(st, &cs);
    reduce_rows_block(partials, rows_of(sel, st), sums);           // (its barrier also publishes the snapshot)
    __syncthreads();
    if (stamp && threadIdx.x == 0) cs.t_acc_start = t_start;       // the search + accumulate part ended where this launch began
    if (threadIdx.x < NSUMS && sums_out) sums_out[threadIdx.x] = sums[threadIdx.x];
    solve_update_block(st, &cs, sums, hist, todo_count);
}

// the same launch for the plane metric: rows of NSUMS_PLANE, the 6 x 6 solve, the shared tail.  (Its accumulation is always a
// launch of its own, which stamps the end of the search.)
__global__ __launch_bounds__(RED_THREADS) void k_reduce_solve_update_plane(DevState *__restrict__ st, const double *__restrict__ partials,
                                                                           int n_rows, double *__restrict__ sums_out,
                                                                           StepRecord *__restrict__ hist, int *__restrict__ todo_count)
{
    __shared__ double sums[NSUMS_PLANE];
    __shared__ DevState cs;
    snapshot_state(st, &cs);
    reduce_rows_block<NSUMS_PLANE>(partials, n_rows, sums);        // (its barrier also publishes the snapshot)
    __syncthreads();
    if (threadIdx.x < NSUMS_PLANE && sums_out) sums_out[threadIdx.x] = sums[threadIdx.x];
    solve_update_block<true>(st, &cs, sums, hist, todo_count);
}
#endif  // !OA_FAMILY_TU

// ------------------------------------------------------------------------------------------------
// multi-device exchange (oa_create_multi): the per-iteration all-gather of the OA_NSUMS partial sums through
// mailboxes.  Two placements (oa_icp.hip picks): DEVICE -- every rank owns an inbox in its own HBM (fine-grained,
// peer-mapped); a post is a remote write into every rank's inbox over xGMI and every rank polls local memory -- or
// HOST -- one box in pinned, portable, device-mapped host memory (fallback when peer access is not available).
// box[parity][rank] holds rank's sums of sequence number `seq` (parity = seq & 1, seq = DevState::seq_base + n + 1);
// every device adds the world's posts in RANK ORDER, so all devices solve from bitwise identical sums and end with
// identical matrices -- no broadcast.  Two parities suffice: rank A can post iteration k + 2 only after its own solve
// of iteration k + 1, which needed rank B's post of k + 1, which B enqueued after its solve of iteration k had read
// A's post of k (from B's own inbox, in the device placement).
// ------------------------------------------------------------------------------------------------
struct MailSlot {
    double sums[NSUMS];
    unsigned long long seq;          // sequence number of the sums above (0 = never written)
    unsigned long long pad[7];       // 256 B per slot: a slot never shares a line with another rank's
};
constexpr int STATUS_EXCHANGE = -9;  // OA_E_RCCL: a rank's post did not arrive in time

// test hook (OA_FAULT_STALL_RANK): the stream stops here until the host releases it -- or for max_ticks of wall_clock64 at
// most, so that no test can hang a GPU
// oa_measure_valu_ceiling: VALU_BURN_CHAINS independent v_fma_f32 chains per lane, `iters` times; workgroup 0's first wave reads
// the shader clock and the constant-rate clock at both ends (clk[0] += shader cycles, clk[1] += wall_clock64 ticks)
constexpr int VALU_BURN_CHAINS = 16;
// OP 0: v_min3_f32, the half-rate class of gfx950 (v_min_f32, v_min3_f32, v_cmp_*_f32: tools/valu_rates.hip) that a third of
// k_nn_search_sorted's instructions belong to; OP 1: v_add_f32, two sources -- one wave-instruction per SIMD every two cycles,
// the issue rate itself
template <int OP>
__global__ __launch_bounds__(256) void k_valu_burn(float *__restrict__ sink, float a, float b, int iters, unsigned long long *__restrict__ clk)
{
    float acc[VALU_BURN_CHAINS];
#pragma unroll
    for (int i = 0; i < VALU_BURN_CHAINS; ++i) acc[i] = (float)threadIdx.x + (float)i;
    const unsigned long long c0 = (unsigned long long)__builtin_readcyclecounter(), w0 = wall_clock64();
    for (int it = 0; it < iters; it += 4) {                          // (64 instructions per trip: the loop's own scalar work stays below 3 %)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int i = 0; i < VALU_BURN_CHAINS; ++i) {
                if (OP == 0) asm volatile("v_min3_f32 %0, %0, %1, %2" : "+v"(acc[i]) : "v"(a), "v"(b));
                else asm volatile("v_add_f32 %0, %0, %1" : "+v"(acc[i]) : "v"(b));
            }
        }
    }
    const unsigned long long c1 = (unsigned long long)__builtin_readcyclecounter(), w1 = wall_clock64();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < VALU_BURN_CHAINS; ++i) t += acc[i];
    sink[(size_t)blockIdx.x * 256 + threadIdx.x] = t;
    if (blockIdx.x == 0 && threadIdx.x == 0) { clk[0] = c1 - c0; clk[1] = w1 - w0; }
}

#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
__global__ void k_fault_stall(const int32_t *release, unsigned long long max_ticks)
{
    if (threadIdx.x != 0) return;
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load(release, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) == 0) {
        if (wall_clock64() - t0 > max_ticks) break;
        __builtin_amdgcn_s_sleep(32);
    }
}

// step 1 on every device: fixed-order reduction of its per-workgroup partials, posted to the mailbox(es).
// dests[0..n_dest): the mailboxes this rank writes its slot of.  Host mailbox: one (the shared pinned box).  Device
// mailboxes: one inbox per rank, each in that rank's own HBM and peer-mapped -- a post is `world` remote writes of
// 200 B that travel over xGMI (PUSH model: every rank later polls its OWN memory).  skip != 0: fault injection
// (OA_FAULT_SKIP_POST_RANK), this rank's sums never arrive and the world's gather kernels run into their time limit.
__global__ __launch_bounds__(RED_THREADS) void k_reduce_post(const DevState *__restrict__ st, const double *__restrict__ partials,
                                                             RowSel sel, MailSlot *const *__restrict__ dests, int n_dest, int rank,
                                                             int world, int skip, unsigned long long *__restrict__ stamp)
{
    if (stamp && threadIdx.x == 0) *stamp = wall_clock64();
    if (st->halt || skip) return;
    __shared__ double sums[NSUMS];
    reduce_rows_block(partials, rows_of(sel, st), sums);
    __syncthreads();
    const unsigned long long seq = st->seq_base + (unsigned long long)st->n + 1ull;
    const size_t slot_ix = (size_t)(seq & 1ull) * world + rank;
    for (int e = threadIdx.x; e < n_dest * 32; e += RED_THREADS) {   // 32 threads per destination, all destinations in flight
        const int d = e >> 5, k = e & 31;
        if (k < NSUMS) __hip_atomic_store(&dests[d][slot_ix].sums[k], sums[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __threadfence_system();
    __syncthreads();
    for (int d = threadIdx.x; d < n_dest; d += RED_THREADS)
        __hip_atomic_store(&dests[d][slot_ix].seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (threadIdx.x == 0) const_cast<DevState *>(st)->t_xchg_start = wall_clock64();
}

// step 2 on every device: wait for the world's posts of this iteration (in this rank's mailbox), add them in rank
// order, solve + update.  Lane r waits for rank r (world <= 64).  The wait is bounded (timeout_ticks of wall_clock64):
// a rank that never posts -- its device faulted -- ends the loop with STATUS_EXCHANGE instead of hanging this one.
__global__ __launch_bounds__(128) void k_gather_solve_update(DevState *__restrict__ st, MailSlot *box, int world,
                                                            double *__restrict__ sums_out, StepRecord *__restrict__ hist,
                                                            int *__restrict__ todo_count, unsigned long long timeout_ticks)
{
    __shared__ double sums[NSUMS];
    __shared__ int arrived;
    __shared__ DevState cs;
    snapshot_state(st, &cs);
    __syncthreads();
    const bool live = cs.halt == 0;
    if (live) {
        const unsigned long long seq = cs.seq_base + (unsigned long long)cs.n + 1ull;
        MailSlot *row = box + (size_t)(seq & 1ull) * world;
        if (threadIdx.x == 0) arrived = 1;
        __syncthreads();
        if ((int)threadIdx.x < world) {
            const unsigned long long t0 = wall_clock64();
            while (__hip_atomic_load(&row[threadIdx.x].seq, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != seq) {
                if (wall_clock64() - t0 > timeout_ticks) { arrived = 0; break; }
                __builtin_amdgcn_s_sleep(4);
            }
        }
        __syncthreads();
        if (arrived && threadIdx.x < NSUMS) {
            double t = __hip_atomic_load(&row[0].sums[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            for (int r = 1; r < world; ++r)
                t += __hip_atomic_load(&row[r].sums[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            sums[threadIdx.x] = t;
            if (sums_out) sums_out[threadIdx.x] = t;
        }
        __syncthreads();
    }
    if (live && !arrived) {                                         // (uniform: `arrived` is shared, read after the barrier)
        if (threadIdx.x == 0) {
            if (todo_count) { todo_count[0] = 0; todo_count[1] = 0; }
            st->status = STATUS_EXCHANGE;
            st->halt = 1;
            if (st->host_halt) { st->host_halt[0] = 1; __threadfence_system(); }
        }
        return;
    }
    solve_update_block(st, &cs, sums, hist, todo_count, live ? wall_clock64() : 0ull);   // (the wait above is over: the world's sums are in hand)
}

// ------------------------------------------------------------------------------------------------
// ordered compaction for make_pairs' A, B outputs (functions/general.py:313-321)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_block_counts(const unsigned char *__restrict__ valid, int ns, int *__restrict__ counts)
{
    __shared__ int wsum[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool v = (i < ns) && valid[i];
    const unsigned long long m = __ballot(v);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// single block exclusive scan of counts[n] -> offsets[n], total in offsets[n]
__global__ __launch_bounds__(1024) void k_scan_counts(const int *__restrict__ counts, int n, long long *__restrict__ offsets)
{
    __shared__ long long wtot[16];
    __shared__ long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        long long v = (i < n) ? counts[i] : 0;
        long long x = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const long long y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        if (lane == 63) wtot[wave] = x;
        __syncthreads();
        long long wpre = 0;
        for (int w = 0; w < wave; ++w) wpre += wtot[w];
        long long tot = 0;
        for (int w = 0; w < 16; ++w) tot += wtot[w];
        const long long c = carry;
        if (i < n) offsets[i] = c + wpre + x - v;
        __syncthreads();
        if (threadIdx.x == 0) carry = c + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[n] = carry;
}

__global__ __launch_bounds__(256) void k_scatter_pairs(const unsigned char *__restrict__ valid, int ns,
                                                       const float4 *__restrict__ src4, const float *__restrict__ b,
                                                       const long long *__restrict__ offsets, long long cap,
                                                       double *__restrict__ A, double *__restrict__ B,
                                                       const int *__restrict__ members, long long begin,
                                                       int *__restrict__ pos)
{
    // pos (optional): the pair's position in the WHOLE selection -- members[i] for a spatial shard, begin + i for a
    // contiguous one -- so that the shards of a multi-device context can be merged back into vlist order
    __shared__ int wsum[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool v = (i < ns) && valid[i];
    const unsigned long long m = __ballot(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    if (!v) return;
    int pre = __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pre += wsum[w];
    const long long k = offsets[blockIdx.x] + pre;
    if (k >= cap) return;
    const float4 p = src4[i];
    A[k] = (double)p.x; A[cap + k] = (double)p.y; A[2 * cap + k] = (double)p.z;
    B[k] = (double)b[3ll * i]; B[cap + k] = (double)b[3ll * i + 1]; B[2 * cap + k] = (double)b[3ll * i + 2];
    if (pos) pos[k] = members ? members[i] : (int)(begin + i);
}
#endif  // !OA_FAMILY_TU

#endif  // __HIPCC__

}  // namespace oa
