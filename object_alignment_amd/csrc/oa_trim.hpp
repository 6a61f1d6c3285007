// oa_trim.hpp -- Trimmed ICP (EXTENSION, oa_set_trim): every step keeps only its best pairs, the share fixed (Chetverikov et al.
// 2002) or estimated by the step itself (fractional ICP, Phillips, Liu and Tomasi 2007).
//
// The contract (include/oa_icp.h):
//   The candidates of a step are the K_q pairs that would be counted in K and carry a vertex weight > 0 -- k_residual_keys' keys
//   other than RKEY_NONE; with oa_set_reciprocal on, the pairs that passed it.  Each has the float32-rounded residual r the losses
//   use (point: the world-space pair distance; plane and symmetric: s |n . (a - b)|; GICP: s sqrt(e^T W e)); its key is the bits of r.
//     - fixed share f:     k = clamp(ceil(f K_q), min(3, K_q), K_q), the cut q = the k-th smallest r.
//     - estimated share:   S_j = sum_{i <= j} (double)r_(i)^2 over the sorted residuals, J(j) = S_j j^-(1 + 2 lambda);
//                          k = the smallest j in [k_min, K_q] that minimises J, k_min = clamp(ceil(f_min K_q), min(3, K_q), K_q);
//                          q = r_(k).
//     - a candidate stays iff r <= q (float32; ties stay, so the verdict does not depend on slot order); a slot that is no
//       candidate keeps the verdict it had.  K_q = 0: q = 0, nothing trimmed.
//
// How: the verdict is the reciprocal check's byte per slot (PairTest<true>::recip_ok), so the accumulation behind a trimmed step
// is the existing RECIP = true instantiation of whatever kernel the step would run -- no accumulation kernel knows about trimming.
// The launches of a step, all on the loop's stream, no host round trip, no float atomics, no workgroup waiting for another:
//   (bytes := 1 unless k_recip_check has just written them; the select's histograms := 0)
//   k_residual_keys<PLANE, RECIP> / k_residual_keys_gicp<RECIP> / k_residual_keys_symm<RECIP>      the keys (+ the select's level-0 counts)
//   fixed:      k_dev_select_scan 0, _hist 1, _scan 1, _hist 2, _scan 2 (oa_deviation.hpp: the radix select of oa_set_robust_auto
//               with its state outside DevState -- DevTrim::sel, so both selections can run in one step)
//   estimated:  sort_order over all 32 key bits (oa_sort.hpp; RKEY_NONE sorts last) + k_gather_int -> the sorted keys
//               k_trim_tile_sums    per tile of TRIM_TILE sorted keys the sum of r^2, fp64, in a fixed order
//               k_trim_tile_bases   one workgroup: exclusive scan of the tile sums in tile order; K_q (the first RKEY_NONE), k_min
//               k_trim_apply        per tile: S_j for its ranks, J(j), one (J, j) minimum per tile
//               k_trim_argmin       one workgroup: the minimum over the tiles, the lowest j winning ties -> k, q
//   k_trim_verdict   one thread per slot: key != RKEY_NONE and key > q -> byte 0; survivors counted with integer atomics
// A halted loop (DevState::halt): the keys kernel and the k_trim_* launches return at once; the select's launches then see no
// counts (K_q = 0) and return after their first line; k_trim_verdict alone publishes the step's figures, so a halted step
// never overwrites the last real one's.
#pragma once
#include "oa_kernels.hpp"
#include "oa_deviation.hpp"            // DevSelect

namespace oa {

struct DevTrim {                          // the trim's state between its launches, and what the host reads back
    DevSelect sel;                        // fixed share: the select's state (p = the fraction, k_min = 3); either mode: kq = K_q, q = the cut
    double lambda, fraction_min;          // estimated share
    uint32_t k_min, k;                    // estimated share: the lowest rank that competes; the rank chosen (0: K_q = 0)
    uint32_t running, done;               // k_trim_verdict: survivors counted so far, workgroups that have finished
    uint32_t stat_kq, stat_kept;          // the last step that ran: candidates, survivors ...
    double stat_q;                        // ... and its cut (0 when K_q = 0)
};

struct TrimTileMin {                      // the smallest J of a tile's ranks and the lowest rank that attains it (j = 0: no rank competed)
    double J;
    unsigned long long j;
};

constexpr int TRIM_THREADS = 256, TRIM_ITEMS = 8, TRIM_TILE = TRIM_THREADS * TRIM_ITEMS;
constexpr int TRIM_BASE_THREADS = 1024;
constexpr int TRIM_VERDICT_MAX_BLOCKS = 2048;
constexpr long long TRIM_AUTO_MAX = 8388608;    // the estimated share: the weighted loop's capacity (PLANE_MAX_BLOCKS * WEIGHTED_THREADS)
inline int trim_tiles(long long n) { return (int)((n + TRIM_TILE - 1) / TRIM_TILE); }

#if defined(__HIPCC__)

// The GICP instance of k_residual_keys (oa_kernels.hpp): the residual k_pair_accumulate_gicp hands to robust_psi, formed exactly
// as that kernel forms it -- pair_fetch<false, true> (read-only), plane_normal for n_b, the slot's source normal normalised in
// the same order, gicp_weight, e^T W e -- as the bits of (float)(res_scale sqrt(max(rr, 0))); RKEY_NONE for a slot without a pair
// counted in K or with vertex weight 0.  Launched like the accumulation (plane_threads / plane_blocks).
template <bool RECIP>
__global__ __launch_bounds__(PLANE_THREADS) void k_residual_keys_gicp(const DevState *__restrict__ st, const float4 *__restrict__ src4, int ns,
                                                                  const float *__restrict__ tgt_xyz,
                                                                  const unsigned long long *__restrict__ keys,
                                                                  const float4 *__restrict__ win, const float4 *__restrict__ tri9,
                                                                  PairTest<RECIP> nrm, const float *__restrict__ plane_tn,
                                                                  const float *__restrict__ src_n, const float *__restrict__ w_slot,
                                                                  uint32_t *__restrict__ rkeys, uint32_t *__restrict__ hist,
                                                                  unsigned long long *__restrict__ t_acc_start)
{
    __shared__ uint32_t bins[SEL_BINS];
    if (t_acc_start && blockIdx.x == 0 && threadIdx.x == 0) *t_acc_start = wall_clock64();   // ~ the end of the search
    if (st->halt) return;
    sel_clear(bins);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t rkey = RKEY_NONE;
    if (i < ns) {
        PairFetch f;
        if (pair_fetch<false, true, RECIP>(st, src4, i, tgt_xyz, keys, nullptr, win, tri9, nrm, plane_tn, st->thresh, f)) {
            double nx = 0.0, ny = 0.0, nz = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
            bool valid = plane_normal(st, f.tn, nx, ny, nz);
            if (valid) {
                const double s0 = (double)src_n[3ll * i], s1 = (double)src_n[3ll * i + 1], s2 = (double)src_n[3ll * i + 2];
                const double n2 = (s0 * s0 + s1 * s1) + s2 * s2;
                valid = (n2 > 0.0) && (n2 < INFINITY);
                const double inv = 1.0 / sqrt(n2);
                sx = s0 * inv; sy = s1 * inv; sz = s2 * inv;
            }
            if (valid && w_slot) valid = w_slot[i] > 0.f;
            if (valid) {
                const double pvx = st->pivot[0], pvy = st->pivot[1], pvz = st->pivot[2];
                const double a0 = (double)f.p.x - pvx, a1 = (double)f.p.y - pvy, a2 = (double)f.p.z - pvz;
                const double e0 = a0 - ((double)f.bx - pvx), e1 = a1 - ((double)f.by - pvy), e2 = a2 - ((double)f.bz - pvz);
                double W[6];
                gicp_weight(st->gicp_eps, sx, sy, sz, nx, ny, nz, W);
                const double u0 = (W[0] * e0 + W[1] * e1) + W[2] * e2, u1 = (W[1] * e0 + W[3] * e1) + W[4] * e2, u2 = (W[2] * e0 + W[4] * e1) + W[5] * e2;
                const double rr = (e0 * u0 + e1 * u1) + e2 * u2;
                rkey = (uint32_t)__float_as_int((float)(st->res_scale * sqrt(fmax(rr, 0.0))));
            }
        }
        rkeys[i] = rkey;
    }
    sel_count(bins, rkey != RKEY_NONE, sel_digit(rkey, 0));
    sel_flush(bins, hist);
}

// The symmetric metric's instance: the residual k_pair_accumulate_symm hands to robust_psi, formed exactly as that kernel forms
// it -- pair_fetch<false, true> (read-only), plane_normal for n_b, symm_source_normal, symm_row -- as the bits of
// (float)(res_scale |r|).  Serves the trim (RECIP = true) and oa_set_robust_auto (either RECIP).
template <bool RECIP>
__global__ __launch_bounds__(PLANE_THREADS) void k_residual_keys_symm(const DevState *__restrict__ st, const float4 *__restrict__ src4, int ns,
                                                                  const float *__restrict__ tgt_xyz,
                                                                  const unsigned long long *__restrict__ keys,
                                                                  const float4 *__restrict__ win, const float4 *__restrict__ tri9,
                                                                  PairTest<RECIP> nrm, const float *__restrict__ plane_tn,
                                                                  const float *__restrict__ src_n, const float *__restrict__ w_slot,
                                                                  uint32_t *__restrict__ rkeys, uint32_t *__restrict__ hist,
                                                                  unsigned long long *__restrict__ t_acc_start)
{
    __shared__ uint32_t bins[SEL_BINS];
    if (t_acc_start && blockIdx.x == 0 && threadIdx.x == 0) *t_acc_start = wall_clock64();   // ~ the end of the search
    if (st->halt) return;
    sel_clear(bins);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t rkey = RKEY_NONE;
    if (i < ns) {
        PairFetch f;
        if (pair_fetch<false, true, RECIP>(st, src4, i, tgt_xyz, keys, nullptr, win, tri9, nrm, plane_tn, st->thresh, f)) {
            double nx = 0.0, ny = 0.0, nz = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
            bool valid = plane_normal(st, f.tn, nx, ny, nz);
            if (valid) valid = symm_source_normal(src_n, i, sx, sy, sz);
            if (valid && w_slot) valid = w_slot[i] > 0.f;
            if (valid) {
                const double pvx = st->pivot[0], pvy = st->pivot[1], pvz = st->pivot[2];
                double j[6], r;
                symm_row((double)f.p.x - pvx, (double)f.p.y - pvy, (double)f.p.z - pvz, (double)f.bx - pvx, (double)f.by - pvy, (double)f.bz - pvz,
                         sx, sy, sz, nx, ny, nz, j, r);
                rkey = (uint32_t)__float_as_int((float)(st->res_scale * fabs(r)));
            }
        }
        rkeys[i] = rkey;
    }
    sel_count(bins, rkey != RKEY_NONE, sel_digit(rkey, 0));
    sel_flush(bins, hist);
}

#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)

// inclusive scan of one double per thread over the workgroup, in a fixed order (the wave's shuffles, then the waves in order);
// `total` = the workgroup's sum.  scan_block_ll's shape (oa_sort.hpp).
__device__ __forceinline__ double trim_block_scan(double v, double *wave_tot, double &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const double t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
    if (lane == 63) wave_tot[w] = v;
    __syncthreads();
    double before = 0.0;
    total = 0.0;
    for (int k = 0; k < nw; ++k) { const double t = wave_tot[k]; if (k < w) before += t; total += t; }
    __syncthreads();
    return v + before;
}

// (double)r^2 of a sorted key: exact in fp64; the RKEY_NONE tail adds nothing
__device__ __forceinline__ double trim_sq(uint32_t key)
{
    const double r = (double)__uint_as_float(key);
    return key != RKEY_NONE ? r * r : 0.0;
}

__global__ __launch_bounds__(TRIM_THREADS) void k_trim_tile_sums(const DevState *__restrict__ st, const uint32_t *__restrict__ sorted, int ns,
                                                                 double *__restrict__ tile_sums)
{
    __shared__ double wave_tot[TRIM_THREADS / 64];
    if (st->halt) return;
    const long long base = (long long)blockIdx.x * TRIM_TILE + (long long)threadIdx.x * TRIM_ITEMS;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < TRIM_ITEMS; ++r) if (base + r < ns) s += trim_sq(sorted[base + r]);
    double total;
    (void)trim_block_scan(s, wave_tot, total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// one workgroup: the tile sums become the tiles' bases (exclusive, in tile order); K_q = the position of the first RKEY_NONE
// among the sorted keys, and the lowest rank that competes
__global__ __launch_bounds__(TRIM_BASE_THREADS) void k_trim_tile_bases(const DevState *__restrict__ st, DevTrim *__restrict__ tr,
                                                                       const uint32_t *__restrict__ sorted, int ns,
                                                                       double *__restrict__ tile_sums, int n_tiles)
{
    __shared__ double wave_tot[TRIM_BASE_THREADS / 64];
    if (st->halt) return;
    double carry = 0.0;
    for (int base = 0; base < n_tiles; base += TRIM_BASE_THREADS) {
        const int i = base + threadIdx.x;
        const double v = i < n_tiles ? tile_sums[i] : 0.0;
        double total;
        const double incl = trim_block_scan(v, wave_tot, total);
        if (i < n_tiles) tile_sums[i] = carry + (incl - v);
        carry += total;
    }
    if (threadIdx.x == 0) {
        int lo = 0, hi = ns;                                         // the first position whose key is RKEY_NONE (the keys are sorted)
        while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (sorted[mid] != RKEY_NONE) lo = mid + 1; else hi = mid; }
        const uint32_t kq = (uint32_t)lo;
        const uint32_t three = kq < 3u ? kq : 3u;
        double k = ceil(tr->fraction_min * (double)kq);
        k = k < (double)three ? (double)three : (k > (double)kq ? (double)kq : k);
        tr->sel.kq = kq;
        tr->k_min = (uint32_t)k;
    }
}

// lexicographic minimum of (J, j) over the wave, every lane gets it
__device__ __forceinline__ void trim_wave_min(double &J, unsigned long long &j)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double oJ = __shfl_xor(J, o, 64);
        const unsigned long long oj = __shfl_xor(j, o, 64);
        if (oJ < J || (oJ == J && oj < j)) { J = oJ; j = oj; }
    }
}

constexpr unsigned long long TRIM_NO_RANK = ~0ull;

// S_j for the tile's ranks (the thread's items in order on top of everything before them), J(j) = S_j j^-(1 + 2 lambda) for the
// ranks in [k_min, K_q], and the tile's (J, j) minimum.  Rank j = position + 1: the candidates lead the sorted keys.
__global__ __launch_bounds__(TRIM_THREADS) void k_trim_apply(const DevState *__restrict__ st, const DevTrim *__restrict__ tr,
                                                             const uint32_t *__restrict__ sorted, int ns, const double *__restrict__ tile_bases,
                                                             TrimTileMin *__restrict__ tile_min)
{
    __shared__ double wave_tot[TRIM_THREADS / 64];
    __shared__ double s_J[TRIM_THREADS / 64];
    __shared__ unsigned long long s_j[TRIM_THREADS / 64];
    if (st->halt) return;
    const long long base = (long long)blockIdx.x * TRIM_TILE + (long long)threadIdx.x * TRIM_ITEMS;
    const unsigned long long k_min = tr->k_min, kq = tr->sel.kq;
    const double expo = -(1.0 + 2.0 * tr->lambda);
    double v[TRIM_ITEMS], s = 0.0;
#pragma unroll
    for (int r = 0; r < TRIM_ITEMS; ++r) { v[r] = base + r < ns ? trim_sq(sorted[base + r]) : 0.0; s += v[r]; }
    double total;
    double run = (trim_block_scan(s, wave_tot, total) - s) + tile_bases[blockIdx.x];
    double bestJ = INFINITY;
    unsigned long long bestj = TRIM_NO_RANK;
#pragma unroll
    for (int r = 0; r < TRIM_ITEMS; ++r) {
        run += v[r];
        const unsigned long long j = (unsigned long long)(base + r) + 1ull;
        if (j >= k_min && j <= kq) {
            const double J = run * pow((double)j, expo);
            if (J < bestJ || bestj == TRIM_NO_RANK) { bestJ = J; bestj = j; }     // (ascending j: the first minimum stays)
        }
    }
    trim_wave_min(bestJ, bestj);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { s_J[w] = bestJ; s_j[w] = bestj; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < TRIM_THREADS / 64; ++k)
            if (s_J[k] < bestJ || (s_J[k] == bestJ && s_j[k] < bestj)) { bestJ = s_J[k]; bestj = s_j[k]; }
        tile_min[blockIdx.x] = TrimTileMin{ bestJ, bestj };
    }
}

// one workgroup: the minimum over the tiles (the lowest j winning ties) -> k and the cut q = r_(k)
__global__ __launch_bounds__(TRIM_THREADS) void k_trim_argmin(const DevState *__restrict__ st, DevTrim *__restrict__ tr,
                                                              const uint32_t *__restrict__ sorted, const TrimTileMin *__restrict__ tile_min, int n_tiles)
{
    __shared__ double s_J[TRIM_THREADS / 64];
    __shared__ unsigned long long s_j[TRIM_THREADS / 64];
    if (st->halt) return;
    double bestJ = INFINITY;
    unsigned long long bestj = TRIM_NO_RANK;
    for (int t = threadIdx.x; t < n_tiles; t += TRIM_THREADS) {
        const TrimTileMin m = tile_min[t];
        if (m.J < bestJ || (m.J == bestJ && m.j < bestj)) { bestJ = m.J; bestj = m.j; }
    }
    trim_wave_min(bestJ, bestj);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { s_J[w] = bestJ; s_j[w] = bestj; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < TRIM_THREADS / 64; ++k)
            if (s_J[k] < bestJ || (s_J[k] == bestJ && s_j[k] < bestj)) { bestJ = s_J[k]; bestj = s_j[k]; }
        const uint32_t kq = tr->sel.kq;
        if (kq == 0u || bestj == TRIM_NO_RANK || bestj > (unsigned long long)kq) { tr->k = 0u; tr->sel.q = 0.0; }
        else { tr->k = (uint32_t)bestj; tr->sel.q = (double)__uint_as_float(sorted[bestj - 1ull]); }
    }
}

// key != RKEY_NONE and key > the cut's key -> the slot's verdict byte becomes 0 (non-negative floats order as their bits).  The
// survivors are counted with an integer atomic -- the total does not depend on the order -- and the last workgroup to finish
// publishes the step's figures and clears the running words for the next step (k_recip_check's scheme).
__global__ __launch_bounds__(TRIM_THREADS) void k_trim_verdict(const DevState *__restrict__ st, DevTrim *__restrict__ tr,
                                                               const uint32_t *__restrict__ rkeys, int ns, unsigned char *__restrict__ ok)
{
    if (st->halt) return;
    const uint32_t kq = tr->sel.kq;
    const uint32_t qbits = kq ? (uint32_t)__float_as_int((float)tr->sel.q) : 0u;
    unsigned kept = 0;
    for (long long i = (long long)blockIdx.x * TRIM_THREADS + threadIdx.x; i < ns; i += (long long)gridDim.x * TRIM_THREADS) {
        const uint32_t key = rkeys[i];
        if (key == RKEY_NONE) continue;
        if (kq && key > qbits) ok[i] = 0;
        else ++kept;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += (unsigned)__shfl_xor((int)kept, o, 64);
    if ((threadIdx.x & 63) == 0 && kept) atomicAdd(&tr->running, kept);
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned done = atomicAdd(&tr->done, 1u);
        if (done == gridDim.x - 1) {                                // the last workgroup: every other one's count is in
            __threadfence();
            tr->stat_kept = atomicExch(&tr->running, 0u);
            tr->stat_kq = kq;
            tr->stat_q = kq ? (double)__uint_as_float(qbits) : 0.0;
            atomicExch(&tr->done, 0u);
        }
    }
}

#endif  // !OA_FAMILY_TU
#endif  // __HIPCC__
}  // namespace oa
