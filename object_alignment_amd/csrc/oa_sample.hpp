// oa_sample.hpp -- normal-space sampling (oa_normal_space_sample) and the 6 x 6 constraint analysis of a selection (oa_stability),
// DESIGN 3.21.  Plain kernels, compiled once in the host translation unit (oa_icp.hip includes this file after oa_sort.hpp).
//
// oa_normal_space_sample (Rusinkiewicz & Levoy 2001, 3.1: bucket the normals, draw evenly across the buckets):
//   k_nss_keys      per point its bin (-1: not eligible), the bin as a sort key (the ineligible ones sort last) and the hash key
//   (sort_order)    by hash, then stably by bin: every bin's members stand together, in hash order
//   k_nss_hist      the bins' member counts: an LDS histogram per workgroup, added to the global one (integer atomics)
//   k_nss_level     ONE workgroup: the level t, the remainder r, every bin's share and its first sorted position
//   k_nss_flag      sorted position j -> flag[point] = (j - start[bin] < share[bin])
//   (scan_counts_ll) and k_nss_compact: the flagged points in ascending index order
// No float arithmetic decides anything but a point's own bin, and no float is ever added to another: two calls give the same bits.
//
// oa_stability (Gelfand et al. 2003: C = sum v v^T, v = [q x n ; n]) -- three passes over the used points, each
//   k_stab_accum<PHASE>   per workgroup the partial sums of the pass  (0: x, y, z;  1: |p - c|;  2: the 21 products v_i v_j, i <= j)
//   k_stab_join           ONE wave: the partials joined, and what the pass is for -- 0: the centroid c; 1: the scale s = 1 / mean
//                         |p - c|; 2: C, its eigen-decomposition (sym6_jacobi), the order and signs of the vectors, rank and cond
// THE ORDER OF SUMMATION (a function of the input alone: of N, the number of points USED -- n_idx, or n without a list).  Every
// sum is fp64, starts at +0 and has no fused multiply-add and no atomics; a point that is not eligible adds nothing.
//   B = min(STAB_MAX_BLOCKS, ceil(N / STAB_THREADS)) workgroups of STAB_THREADS threads.  Thread g = b STAB_THREADS + t adds the
//   used points at positions g, g + B STAB_THREADS, g + 2 B STAB_THREADS, ... in ascending order.  The 64 sums of a wave are joined
//   by the butterfly t_l = s_l + s_(l ^ 32), then strides 16, 8, 4, 2, 1 likewise; the workgroup's partial is
//   ((w_0 + w_1) + w_2) + w_3 of its four waves' sums.  k_stab_join: lane l of one wave adds the partials l, l + 64, l + 128, ...
//   in ascending order, and the 64 lane sums are joined by the same butterfly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "oa_kernels.hpp"               // sym6_jacobi, sym6_index, PLANE_EIG_CUT
#include "oa_sort.hpp"                  // scan_block_ll

namespace oa {

constexpr int NSS_THREADS = 256;
constexpr int NSS_MAX_GRID = 32;                                    // G: cells per edge of a cube face
constexpr int NSS_MAX_BINS = 6 * NSS_MAX_GRID * NSS_MAX_GRID;       // 6144 ints: the LDS histogram of k_nss_hist
constexpr int NSS_HIST_BLOCKS = 256;
constexpr int NSS_LEVEL_THREADS = 1024;
constexpr int NSS_LEVEL_BPT = NSS_MAX_BINS / NSS_LEVEL_THREADS;     // bins per thread of k_nss_level
static_assert(NSS_LEVEL_BPT * NSS_LEVEL_THREADS == NSS_MAX_BINS, "k_nss_level: every bin has a thread");

// what the host reads back, once
struct NssInfo { long long n_eligible, n_out, bins_occupied, level, max_bin_count; };

constexpr int STAB_THREADS = 256;
constexpr int STAB_MAX_BLOCKS = 256;                                // (a fixed constant: part of the summation order)
constexpr int STAB_NT = 21;                                         // the widest pass: the upper triangle of C

struct StabOut {
    double c[3], mean_dist, s;
    long long n_used;
    double C[36], eig[6], vec[36], cond;
    int rank, pad;
};

#if defined(__HIPCC__)

// eligible: three finite components and a squared length (x x + y y) + z z, in fp64, that is finite and > 0
__device__ __forceinline__ bool smp_normal_ok(float x, float y, float z, double &l2)
{
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    l2 = (dx * dx + dy * dy) + dz * dz;
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY && l2 > 0.0 && l2 < (double)INFINITY;
}

// the cell of one face coordinate u in [-1, 1]: min(G - 1, floor((u + 1) (G / 2))).  (|u| <= 1 exactly -- an IEEE quotient of two
// numbers the first of which is not the larger -- so the lower clamp never acts; it keeps an index in range whatever happens.)
__device__ __forceinline__ int nss_cell(double u, int G) { return max(0, min(G - 1, (int)floor((u + 1.0) * (0.5 * (double)G)))); }

// the bin of a normal, -1 when it is not eligible.  a = the axis of the largest |component| (ties: the lowest axis), b, c the next
// two; oriented: face 2 a + (n_a < 0), (u, v) = (n_b, n_c) / |n_a|; unoriented: face a, (u, v) = (n_b, n_c) / n_a -- n and -n share
// a bin.  No square root, no normalisation: three comparisons, two IEEE divisions, two floors.
__device__ __forceinline__ int nss_bin(float x, float y, float z, int G, int unoriented)
{
    double l2;
    if (!smp_normal_ok(x, y, z, l2)) return -1;
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    int a = 0;
    double big = fabs(dx);
    if (fabs(dy) > big) { a = 1; big = fabs(dy); }
    if (fabs(dz) > big) a = 2;
    // (scalars and selects, not arrays: a dynamic index keeps an array in scratch memory)
    const double na = a == 0 ? dx : (a == 1 ? dy : dz), nb = a == 0 ? dy : (a == 1 ? dz : dx), nc = a == 0 ? dz : (a == 1 ? dx : dy);
    const double den = unoriented ? na : fabs(na);
    const int iu = nss_cell(nb / den, G), iv = nss_cell(nc / den, G);
    const int f = unoriented ? a : 2 * a + (na < 0.0 ? 1 : 0);
    return (f * G + iv) * G + iu;
}

#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)

// Launch: NSS_THREADS threads, ceil(n / NSS_THREADS) workgroups.  hash = (uint32)((i ^ seed) * 0x9E3779B1): a bijection of the
// 32-bit index, so no two points of a call share a key.  bin_key: the bin, or n_bins for a point that takes no part.
__global__ __launch_bounds__(NSS_THREADS) void k_nss_keys(const float *__restrict__ nrm, int n, int G, int unoriented, uint32_t seed, int n_bins,
                                                          int *__restrict__ bin, uint32_t *__restrict__ bin_key, uint32_t *__restrict__ hash)
{
    const long long i = (long long)blockIdx.x * NSS_THREADS + threadIdx.x;
    if (i >= n) return;
    const int b = nss_bin(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2], G, unoriented);
    bin[i] = b;
    bin_key[i] = b < 0 ? (uint32_t)n_bins : (uint32_t)b;
    hash[i] = ((uint32_t)i ^ seed) * 0x9E3779B1u;
}

// Launch: NSS_THREADS threads, any number of workgroups; counts[0 .. n_bins) zeroed before.  n_bins <= NSS_MAX_BINS.
__global__ __launch_bounds__(NSS_THREADS) void k_nss_hist(const int *__restrict__ bin, int n, int n_bins, int *__restrict__ counts)
{
    __shared__ int h[NSS_MAX_BINS];
    for (int b = threadIdx.x; b < n_bins; b += NSS_THREADS) h[b] = 0;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * NSS_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * NSS_THREADS) {
        const int b = bin[i];
        if (b >= 0 && b < n_bins) atomicAdd(&h[b], 1);              // (integer counts: the order of the atomics is immaterial)
    }
    __syncthreads();
    for (int b = threadIdx.x; b < n_bins; b += NSS_THREADS)
        if (h[b]) atomicAdd(&counts[b], h[b]);
}

// Launch: ONE workgroup of NSS_LEVEL_THREADS threads; thread t owns the bins t BPT .. t BPT + BPT - 1.
// level t = the largest integer with sum_b min(c_b, t) <= m (m >= n_eligible: every eligible point is given, t = the largest
// count); the remainder r = m - sum_b min(c_b, t) goes one each to the first r bins, in ascending bin id, with c_b > t.
// share[b] = what bin b gives, start[b] = the sorted position of its first member (the exclusive sum of the counts).
__global__ __launch_bounds__(NSS_LEVEL_THREADS) void k_nss_level(const int *__restrict__ counts, int n_bins, long long m, int *__restrict__ share,
                                                                 long long *__restrict__ start, NssInfo *__restrict__ info)
{
    __shared__ long long wave_tot[NSS_LEVEL_THREADS / 64];
    __shared__ int wave_max[NSS_LEVEL_THREADS / 64];
    const int first = threadIdx.x * NSS_LEVEL_BPT;
    int c[NSS_LEVEL_BPT];
    long long mine = 0, occupied = 0;
    int mx = 0;
#pragma unroll
    for (int k = 0; k < NSS_LEVEL_BPT; ++k) {
        c[k] = first + k < n_bins ? counts[first + k] : 0;
        mine += c[k]; occupied += c[k] > 0 ? 1 : 0; mx = max(mx, c[k]);
    }
    long long n_eligible, n_occupied;
    const long long before = scan_block_ll(mine, wave_tot, n_eligible) - mine;       // the members of the bins below this thread's
    (void)scan_block_ll(occupied, wave_tot, n_occupied);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    int max_count = 0;
    for (int k = 0; k < NSS_LEVEL_THREADS / 64; ++k) max_count = max(max_count, wave_max[k]);
    // (everything below is uniform: every thread holds the same totals)
    long long level = max_count, given = n_eligible;
    if (m < n_eligible) {
        long long lo = 0, hi = max_count;                           // sum min(c, lo) <= m < sum min(c, hi)
        while (hi - lo > 1) {
            const long long mid = lo + ((hi - lo) >> 1);
            long long part = 0, total;
#pragma unroll
            for (int k = 0; k < NSS_LEVEL_BPT; ++k) part += min((long long)c[k], mid);
            (void)scan_block_ll(part, wave_tot, total);
            if (total <= m) lo = mid; else hi = mid;
        }
        level = lo;
        long long part = 0;
#pragma unroll
        for (int k = 0; k < NSS_LEVEL_BPT; ++k) part += min((long long)c[k], level);
        (void)scan_block_ll(part, wave_tot, given);
    }
    const long long r = (m < n_eligible ? m : n_eligible) - given;  // 0 <= r < the number of bins above the level
    long long above = 0, all_above;
#pragma unroll
    for (int k = 0; k < NSS_LEVEL_BPT; ++k) above += (long long)c[k] > level ? 1 : 0;
    long long rank = scan_block_ll(above, wave_tot, all_above) - above;              // bins above the level below this thread's
    long long pos = before;
#pragma unroll
    for (int k = 0; k < NSS_LEVEL_BPT; ++k) {
        if (first + k < n_bins) {
            const bool over = (long long)c[k] > level;
            share[first + k] = (int)min((long long)c[k], level) + ((over && rank < r) ? 1 : 0);
            start[first + k] = pos;
            rank += over ? 1 : 0;
            pos += c[k];
        }
    }
    if (threadIdx.x == 0) {
        info->n_eligible = n_eligible; info->bins_occupied = n_occupied; info->level = level; info->max_bin_count = max_count;
        info->n_out = 0;                                            // (k_nss_compact writes the number of rows)
    }
}

// Launch: NSS_THREADS threads, ceil(n / NSS_THREADS) workgroups.  order: the points by (bin, hash); the ineligible ones last.
__global__ __launch_bounds__(NSS_THREADS) void k_nss_flag(const int *__restrict__ order, const int *__restrict__ bin, int n, int n_bins,
                                                          const int *__restrict__ share, const long long *__restrict__ start, int *__restrict__ flag)
{
    const long long j = (long long)blockIdx.x * NSS_THREADS + threadIdx.x;
    if (j >= n) return;
    const int i = order[j];
    if (i < 0 || i >= n) return;                                    // (a permutation of 0 .. n - 1: never taken)
    const int b = bin[i];
    flag[i] = (b >= 0 && b < n_bins && j - start[b] < (long long)share[b]) ? 1 : 0;
}

// off = the exclusive scan of flag (off[n] = the number of rows): the flagged points in ascending index order -- a vlist
__global__ __launch_bounds__(NSS_THREADS) void k_nss_compact(const int *__restrict__ flag, const long long *__restrict__ off, int n, long long cap,
                                                             long long *__restrict__ out, NssInfo *__restrict__ info)
{
    const long long i = (long long)blockIdx.x * NSS_THREADS + threadIdx.x;
    if (i == 0) info->n_out = off[n];
    if (i >= n) return;
    if (flag[i] && off[i] < cap) out[off[i]] = i;
}

// ---- oa_stability -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool stab_fetch(const float *__restrict__ xyz, const float *__restrict__ nrm, long long i, double p[3], double nh[3])
{
    const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
    const float nx = nrm[3 * i], ny = nrm[3 * i + 1], nz = nrm[3 * i + 2];
    double l2;
    if (!smp_normal_ok(nx, ny, nz, l2) || !(fabsf(px) < INFINITY && fabsf(py) < INFINITY && fabsf(pz) < INFINITY)) return false;
    const double inv = 1.0 / sqrt(l2);
    p[0] = (double)px; p[1] = (double)py; p[2] = (double)pz;
    nh[0] = (double)nx * inv; nh[1] = (double)ny * inv; nh[2] = (double)nz * inv;
    return true;
}

// Launch: STAB_THREADS threads, B = min(STAB_MAX_BLOCKS, ceil(n_used / STAB_THREADS)) workgroups (the summation order above).
// idx: the used points (device int64, every entry in 0 .. n - 1, checked by the host), or nullptr for all.  partial: B x STAB_NT.
template <int PHASE>
__global__ __launch_bounds__(STAB_THREADS) void k_stab_accum(const float *__restrict__ xyz, const float *__restrict__ nrm, const long long *__restrict__ idx,
                                                             long long n_used, const StabOut *__restrict__ st, double *__restrict__ partial,
                                                             long long *__restrict__ partial_count)
{
    constexpr int NT = PHASE == 0 ? 3 : (PHASE == 1 ? 1 : STAB_NT);
    __shared__ double red[STAB_THREADS / 64][NT];
    __shared__ long long red_count[STAB_THREADS / 64];
    double acc[NT];
#pragma unroll
    for (int a = 0; a < NT; ++a) acc[a] = 0.0;
    long long count = 0;
    double c[3] = { 0.0, 0.0, 0.0 }, s = 0.0;
    if (PHASE >= 1) { c[0] = st->c[0]; c[1] = st->c[1]; c[2] = st->c[2]; }
    if (PHASE == 2) s = st->s;
    for (long long j = (long long)blockIdx.x * STAB_THREADS + threadIdx.x; j < n_used; j += (long long)gridDim.x * STAB_THREADS) {
        const long long i = idx ? idx[j] : j;
        double p[3], nh[3];
        if (!stab_fetch(xyz, nrm, i, p, nh)) continue;
        ++count;
        if (PHASE == 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) acc[a] += p[a];
        } else if (PHASE == 1) {
            const double dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
            acc[0] += sqrt((dx * dx + dy * dy) + dz * dz);
        } else {
            const double qx = (p[0] - c[0]) * s, qy = (p[1] - c[1]) * s, qz = (p[2] - c[2]) * s;
            const double v[6] = { qy * nh[2] - qz * nh[1], qz * nh[0] - qx * nh[2], qx * nh[1] - qy * nh[0], nh[0], nh[1], nh[2] };
            int k = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b) acc[k++] += v[a] * v[b];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < NT; ++a) acc[a] += __shfl_xor(acc[a], o, 64);
        count += __shfl_xor(count, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < NT; ++a) red[threadIdx.x >> 6][a] = acc[a];
        red_count[threadIdx.x >> 6] = count;
    }
    __syncthreads();
    if (threadIdx.x < NT) {
        const int a = threadIdx.x;
        partial[(size_t)blockIdx.x * STAB_NT + a] = ((red[0][a] + red[1][a]) + red[2][a]) + red[3][a];
    }
    if (threadIdx.x == 0) partial_count[blockIdx.x] = ((red_count[0] + red_count[1]) + red_count[2]) + red_count[3];
}

// Launch: ONE wave.  phase 0: st->c, st->n_used; 1: st->mean_dist, st->s (0 when the mean distance is 0 or not finite);
// 2: st->C, eig (descending; equal ones in the order sym6_jacobi left them), vec (columns, each signed so that its component of
// largest magnitude -- the lowest index on ties -- is positive), rank = the eigenvalues above PLANE_EIG_CUT x the largest (0 when
// s = 0), cond = eig[0] / eig[5], +inf when eig[5] <= 0 or s = 0.
__global__ __launch_bounds__(64) void k_stab_join(const double *__restrict__ partial, const long long *__restrict__ partial_count, int n_blocks, int phase,
                                                  StabOut *__restrict__ st)
{
    __shared__ double sh_s[STAB_NT], sh_A[36], sh_V[36], sh_lam[6];
    __shared__ int sh_used[6];
    const int lane = threadIdx.x;
    const int nt = phase == 0 ? 3 : (phase == 1 ? 1 : STAB_NT);
    double acc[STAB_NT];
#pragma unroll
    for (int a = 0; a < STAB_NT; ++a) acc[a] = 0.0;
    long long count = 0;
    for (int r = lane; r < n_blocks; r += 64) {
#pragma unroll
        for (int a = 0; a < STAB_NT; ++a)
            if (a < nt) acc[a] += partial[(size_t)r * STAB_NT + a];
        count += partial_count[r];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < STAB_NT; ++a) acc[a] += __shfl_xor(acc[a], o, 64);
        count += __shfl_xor(count, o, 64);
    }
    if (phase == 0) {
        if (lane == 0) {
            st->n_used = count;
            const double k = (double)count;
            st->c[0] = count > 0 ? acc[0] / k : 0.0; st->c[1] = count > 0 ? acc[1] / k : 0.0; st->c[2] = count > 0 ? acc[2] / k : 0.0;
        }
        return;
    }
    if (phase == 1) {
        if (lane == 0) {
            const double mean = count > 0 ? acc[0] / (double)count : 0.0;
            st->mean_dist = mean;
            st->s = (mean > 0.0 && mean < (double)INFINITY) ? 1.0 / mean : 0.0;
        }
        return;
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < STAB_NT; ++a) sh_s[a] = acc[a];
    }
    __syncthreads();
    if (lane < 36) {
        const int i = lane / 6, j = lane % 6;
        const double v = sh_s[i <= j ? sym6_index(i, j) : sym6_index(j, i)];
        sh_A[lane] = v;
        st->C[lane] = v;
    }
    __syncthreads();
    sym6_jacobi(sh_A, sh_V, lane < 6 ? lane : 6, lane < 6 ? lane + 1 : 6);
    __syncthreads();
    if (lane != 0) return;
    // (the order lives in LDS: a dynamic index keeps a local array in scratch memory)
    for (int p = 0; p < 6; ++p) sh_used[p] = 0;
    for (int k = 0; k < 6; ++k) {                                   // a stable selection: the largest unused, the lowest column on ties
        int best = -1;
        for (int p = 0; p < 6; ++p)
            if (!sh_used[p] && (best < 0 || sh_A[7 * p] > sh_A[7 * best])) best = p;
        sh_used[best] = 1;
        sh_lam[k] = sh_A[7 * best];
        int rmax = 0;
        for (int r = 1; r < 6; ++r)
            if (fabs(sh_V[6 * r + best]) > fabs(sh_V[6 * rmax + best])) rmax = r;
        const double sgn = sh_V[6 * rmax + best] < 0.0 ? -1.0 : 1.0;
        for (int r = 0; r < 6; ++r) st->vec[6 * r + k] = sgn * sh_V[6 * r + best];
        st->eig[k] = sh_lam[k];
    }
    const bool flat = !(st->s > 0.0);
    const double top = sh_lam[0], low = sh_lam[5];
    int rank = 0;
    for (int k = 0; k < 6; ++k) rank += sh_lam[k] > PLANE_EIG_CUT * top ? 1 : 0;
    st->rank = flat ? 0 : rank;
    st->cond = (flat || !(low > 0.0)) ? (double)INFINITY : top / low;
    st->pad = 0;
}

#endif  // !OA_FAMILY_TU
#endif  // __HIPCC__
}  // namespace oa
