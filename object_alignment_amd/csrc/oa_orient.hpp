// oa_orient.hpp -- one consistent sign for the normals of a point-cloud target (oa_orient_target_normals).
// Hoppe et al. 1992: the minimum spanning forest of the neighbour graph under the weights 1 - |n_i . n_j|, signs handed along
// its edges.  Plain kernels, compiled once in the host translation unit (oa_icp.hip includes this file after oa_sort.hpp).
//
//   k_orient_init     per vertex: eligible or not, its own root (parent = itself, parity 0)
//   k_orient_entries  per entry e = (i, t) of the k-nearest rows: is it an edge {i, j}, its flip bit, and its three sort keys
//                     (weight bits, min(i, j), max(i, j))
//   (sort_order)      three stable passes, hi then lo then weight: ord[p] = the entry at position p of the order (w, lo, hi)
//   k_orient_rank     rank[ord[p]] = p.  Both directions of an edge carry equal keys: whichever stands first names the edge
//   -- a Boruvka round, at most ceil(log2 nt) + 1 of them --
//   k_orient_min      per entry whose ends have different roots: best[root] = min(best[root], rank) for BOTH roots (integer
//                     atomicMin; one per wave where the wave's live lanes share the root)
//   k_orient_hook     per root with an edge (u inside, v outside): parent = root(v), parity = par[u] ^ flip ^ par[v]; when the two
//                     roots chose the same edge the lower root stays.  Reads P, writes Q: nobody sees a half-made forest
//   k_orient_jump     Q[x] = P[x] joined with P[parent(x)], (parent, parity) in ONE word, read from one buffer and written to the
//                     other.  Jump j runs only if jump j - 1 changed a word (the first: if a root was hooked); one that changes
//                     nothing has copied its input, so after the round both buffers are equal and the host need not know how
//                     many jumps ran.  The host reads OrientRound back once per round.
//   -- then --
//   k_orient_label    per root the lowest index of its component, and the extreme squared distance to the seed point
//   k_orient_seed     per root the lowest index among the vertices at that distance
//   k_orient_sign     per root: does its component flip (the seed's parity, and the fp64 sign test at the seed)
//   k_orient_apply    per vertex: flipped = parity ^ component flip; the normal with three sign bits toggled or not
// Every decision is an integer comparison or an fp64 comparison of one vertex's own numbers; atomics are integer min / max / add
// whose results do not depend on the order they arrive in: two calls give the same bits.  No kernel waits for another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oa {

constexpr int ORI_THREADS = 256;
constexpr uint32_t ORI_NONE = 0xFFFFFFFFu;                          // no entry / no edge / no vertex (what hipMemset 0xff leaves)
constexpr uint32_t ORI_W_NONE = 0x3F800001u;                        // the weight key of an entry that is no edge: above 1.0f = 0x3F800000
constexpr int ORI_W_BITS = 30;                                      // ... and still below 2^30: three passes of the sort, not four
constexpr int ORI_MAX_JUMPS = 33;                                   // ceil(log2 nt) + 1 <= 32 for nt < 2^31

// what the host reads back once per round; zeroed before the round
struct OrientRound { int hooked, changed[ORI_MAX_JUMPS + 1]; };
// what the host reads back at the end; zeroed before
struct OrientInfo { unsigned long long n_components, n_left_out, n_flipped; };
struct OrientSeed { int32_t mode, pad; double p[3]; };            // OA_SEED_*, the point

#if defined(__HIPCC__)
#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)

__device__ __forceinline__ bool ori_finite3(float x, float y, float z) { return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY; }

// one add per workgroup of the number of threads for which pred holds (EVERY thread of the workgroup calls this: it is a barrier)
__device__ __forceinline__ void ori_count(bool pred, unsigned long long *cell)
{
    const int n = __syncthreads_count(pred ? 1 : 0);
    if (threadIdx.x == 0 && n) atomicAdd(cell, (unsigned long long)n);
}

// fp64, one rounding per operation: (dx dx + dy dy) + dz dz with d = (double)v - p
__device__ __forceinline__ double ori_dist2(const float *__restrict__ xyz, long long i, const double p[3])
{
    const double dx = __dsub_rn((double)xyz[3 * i], p[0]), dy = __dsub_rn((double)xyz[3 * i + 1], p[1]), dz = __dsub_rn((double)xyz[3 * i + 2], p[2]);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// Launch: ORI_THREADS threads, ceil(nt / ORI_THREADS) workgroups.  Eligible: a finite normal that is not (0, 0, 0), finite coordinates.
__global__ __launch_bounds__(ORI_THREADS) void k_orient_init(const float *__restrict__ xyz, const float *__restrict__ nrm, int nt, uint8_t *__restrict__ elig,
                                                             uint32_t *__restrict__ P)
{
    const long long x = (long long)blockIdx.x * ORI_THREADS + threadIdx.x;
    if (x >= nt) return;
    const float nx = nrm[3 * x], ny = nrm[3 * x + 1], nz = nrm[3 * x + 2];
    elig[x] = (ori_finite3(nx, ny, nz) && (nx != 0.0f || ny != 0.0f || nz != 0.0f) && ori_finite3(xyz[3 * x], xyz[3 * x + 1], xyz[3 * x + 2])) ? 1 : 0;
    P[x] = (uint32_t)x << 1;
}

// Launch: ORI_THREADS threads, ceil(n_ent / ORI_THREADS) workgroups; n_ent = nt k <= 2^31 - 1.
// Entry e = (i = e / k, j = idx[e]) is an edge when j is a vertex other than i, both are eligible and (cap_on) d2[e] <= cap2.
// d = (nx_i nx_j + ny_i ny_j) + nz_i nz_j in float32, one rounding per operation; t = 1 - |d|; w = t > 0 ? t : +0 (a NaN: 0);
// the edge flips iff d < 0.  ent = j | flip << 31, ORI_NONE when the entry is no edge.
__global__ __launch_bounds__(ORI_THREADS) void k_orient_entries(const int32_t *__restrict__ idx, const float *__restrict__ d2, const float *__restrict__ nrm,
                                                                const uint8_t *__restrict__ elig, int nt, int k, long long n_ent, int cap_on, float cap2,
                                                                uint32_t *__restrict__ ent, uint32_t *__restrict__ key_w, uint32_t *__restrict__ key_lo,
                                                                uint32_t *__restrict__ key_hi)
{
    const long long e = (long long)blockIdx.x * ORI_THREADS + threadIdx.x;
    if (e >= n_ent) return;
    const int i = (int)((uint32_t)e / (uint32_t)k), j = idx[e];       // (e < 2^31)
    bool edge = j >= 0 && j < nt && j != i;
    if (edge) edge = elig[i] && elig[j] && (!cap_on || d2[e] <= cap2);
    if (!edge) { ent[e] = ORI_NONE; key_w[e] = ORI_W_NONE; key_lo[e] = 0u; key_hi[e] = 0u; return; }
    const float d = __fadd_rn(__fadd_rn(__fmul_rn(nrm[3 * (long long)i], nrm[3 * (long long)j]), __fmul_rn(nrm[3 * (long long)i + 1], nrm[3 * (long long)j + 1])),
                              __fmul_rn(nrm[3 * (long long)i + 2], nrm[3 * (long long)j + 2]));
    const float t = __fsub_rn(1.0f, fabsf(d));
    const float w = t > 0.0f ? t : 0.0f;
    ent[e] = (uint32_t)j | (d < 0.0f ? 0x80000000u : 0u);
    key_w[e] = __float_as_uint(w);                                   // 0 <= w <= 1: the bits order as the numbers do
    key_lo[e] = (uint32_t)min(i, j);
    key_hi[e] = (uint32_t)max(i, j);
}

// Launch: ORI_THREADS threads, ceil(n_ent / ORI_THREADS) workgroups.  ord: a permutation of 0 .. n_ent - 1.
__global__ __launch_bounds__(ORI_THREADS) void k_orient_rank(const int *__restrict__ ord, long long n_ent, uint32_t *__restrict__ rank)
{
    const long long p = (long long)blockIdx.x * ORI_THREADS + threadIdx.x;
    if (p >= n_ent) return;
    const int e = ord[p];
    if (e >= 0 && e < n_ent) rank[e] = (uint32_t)p;
}

// best[root] = min(best[root], r) for the live lanes.  Where every live lane of the wave has the same root -- the rows of one
// vertex always do, and after the first rounds so do most neighbours in the caller's order -- the wave joins its ranks first and
// one lane asks; a lane whose rank cannot win does not ask at all (best only falls during the launch, and the read goes past
// this CU's L1).  Every lane of the wave calls this.
__device__ __forceinline__ void ori_wave_min(uint32_t *__restrict__ best, uint32_t root, uint32_t r, bool live)
{
    const unsigned long long m = __ballot(live);
    if (!m) return;
    const int first = __ffsll((long long)m) - 1;
    const uint32_t root0 = (uint32_t)__builtin_amdgcn_readlane((int)root, first);
    if (__ballot(live && root != root0) == 0ull) {
        uint32_t v = live ? r : ORI_NONE;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
        if ((int)(threadIdx.x & 63) == first && v < __hip_atomic_load(&best[root0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&best[root0], v);
    } else if (live && r < __hip_atomic_load(&best[root], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        atomicMin(&best[root], r);
    }
}

// the same for a 64-bit minimum (want_max false) or maximum: a component's extreme distance.  At the end every vertex of a
// component has the same root -- one cell for a whole cloud -- so the wave joins first and asks only if it can still win.
__device__ __forceinline__ void ori_wave_extreme(unsigned long long *__restrict__ cell, uint32_t root, unsigned long long v, bool live, bool want_max)
{
    const unsigned long long m = __ballot(live);
    if (!m) return;
    const int first = __ffsll((long long)m) - 1;
    const uint32_t root0 = (uint32_t)__builtin_amdgcn_readlane((int)root, first);
    const bool shared = __ballot(live && root != root0) == 0ull;
    unsigned long long r = live ? v : (want_max ? 0ull : ~0ull);
    if (shared) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(r, o, 64);
            r = want_max ? (other > r ? other : r) : (other < r ? other : r);
        }
    }
    if (shared ? (int)(threadIdx.x & 63) != first : !live) return;
    const uint32_t to = shared ? root0 : root;
    const unsigned long long cur = __hip_atomic_load(&cell[to], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (want_max) { if (r > cur) atomicMax(&cell[to], r); }
    else if (r < cur) atomicMin(&cell[to], r);
}

// Launch: ORI_THREADS threads, ceil(n_ent / ORI_THREADS) workgroups; best[0 .. nt) = ORI_NONE before.  P: every vertex points at
// its root.
__global__ __launch_bounds__(ORI_THREADS) void k_orient_min(const uint32_t *__restrict__ ent, const uint32_t *__restrict__ rank, const uint32_t *__restrict__ P,
                                                            int k, long long n_ent, uint32_t *__restrict__ best)
{
    const long long e = (long long)blockIdx.x * ORI_THREADS + threadIdx.x;
    const uint32_t en = e < n_ent ? ent[e] : ORI_NONE;
    bool live = en != ORI_NONE;
    uint32_t ru = 0u, rv = 0u, r = ORI_NONE;
    if (live) {
        ru = P[(uint32_t)e / (uint32_t)k] >> 1;
        rv = P[en & 0x7FFFFFFFu] >> 1;
        live = ru != rv;
        if (live) r = rank[e];
    }
    ori_wave_min(best, ru, r, live);
    ori_wave_min(best, rv, r, live);
}

// Launch: ORI_THREADS threads, ceil(nt / ORI_THREADS) workgroups.  P: every vertex points at its root (roots at themselves,
// parity 0).  Q[x] = P[x], but for a root that hooks.  st->hooked counts those.
__global__ __launch_bounds__(ORI_THREADS) void k_orient_hook(const uint32_t *__restrict__ P, const uint32_t *__restrict__ best, const int *__restrict__ ord,
                                                             const uint32_t *__restrict__ ent, int nt, int k, long long n_ent, uint32_t *__restrict__ Q,
                                                             OrientRound *__restrict__ st)
{
    const long long x = (long long)blockIdx.x * ORI_THREADS + threadIdx.x;
    const bool in = x < nt;
    const uint32_t w = in ? P[x] : 0u;
    uint32_t out = w;
    const uint32_t b = (in && (w >> 1) == (uint32_t)x) ? best[x] : ORI_NONE;
    if (b != ORI_NONE && (long long)b < n_ent) {
        const int e = ord[b];
        const uint32_t en = (e >= 0 && e < n_ent) ? ent[e] : ORI_NONE;
        const uint32_t a = (uint32_t)e / (uint32_t)k, c = en & 0x7FFFFFFFu;
        if (en != ORI_NONE && c < (uint32_t)nt) {                    // (always: the rank came from an edge)
            const uint32_t pa = P[a], pc = P[c];
            const bool a_inside = (pa >> 1) == (uint32_t)x;
            const uint32_t pu = a_inside ? pa : pc, pv = a_inside ? pc : pa;
            const uint32_t rv = pv >> 1;
            const bool stays = best[rv] == b && (uint32_t)x < rv;    // both roots chose this edge: the lower one stays a root
            if (rv != (uint32_t)x && !stays) out = (rv << 1) | ((pu ^ pv ^ (en >> 31)) & 1u);
        }
    }
    if (in) Q[x] = out;
    const int n = __syncthreads_count(out != w ? 1 : 0);            // (one add per workgroup: in the first round most roots hook)
    if (threadIdx.x == 0 && n) atomicAdd(&st->hooked, n);
}

// Launch: ORI_THREADS threads, ceil(nt / ORI_THREADS) workgroups; jump = 1, 2, ...  dst[x] = (parent of parent, parity to it).
__global__ __launch_bounds__(ORI_THREADS) void k_orient_jump(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, int nt, int jump,
                                                             OrientRound *__restrict__ st)
{
    if (!(jump == 1 ? st->hooked : st->changed[jump - 1])) return;  // (uniform: the launch before wrote it)
    const long long x = (long long)blockIdx.x * ORI_THREADS + threadIdx.x;
    if (x >= nt) return;
    const uint32_t w = src[x], g = src[w >> 1];
    const uint32_t out = (g & ~1u) | ((w ^ g) & 1u);
    dst[x] = out;
    if (out != w) st->changed[jump] = 1;
}

// Launch: ORI_THREADS threads, ceil(nt / ORI_THREADS) workgroups; label[] = ORI_NONE before; dkey[] = all ones (TOWARD: a
// minimum) or 0 (AWAY: a maximum) before.  label[root] = the lowest index of the component; dkey[root] = the bits of the
// extreme fp64 squared distance (they order as the distances do: none is negative).
__global__ __launch_bounds__(ORI_THREADS) void k_orient_label(const uint32_t *__restrict__ P, const uint8_t *__restrict__ elig, const float *__restrict__ xyz,
                                                              int nt, OrientSeed seed, uint32_t *__restrict__ label, unsigned long long *__restrict__ dkey)
{
    const long long x = (long long)blockIdx.x * ORI_THREADS + threadIdx.x;
    const bool live = x < nt && elig[x];
    const uint32_t root = live ? P[x] >> 1 : 0u;
    ori_wave_min(label, root, (uint32_t)x, live);
    if (seed.mode == 0) return;
    const unsigned long long kd = live ? (unsigned long long)__double_as_longlong(ori_dist2(xyz, x, seed.p)) : 0ull;
    ori_wave_extreme(dkey, root, kd, live, seed.mode != 1);
}

// Launch: as k_orient_label, after it; seed_of[] = ORI_NONE before.  seed_of[root] = the lowest index at the extreme distance.
__global__ __launch_bounds__(ORI_THREADS) void k_orient_seed(const uint32_t *__restrict__ P, const uint8_t *__restrict__ elig, const float *__restrict__ xyz,
                                                             int nt, OrientSeed seed, const unsigned long long *__restrict__ dkey, uint32_t *__restrict__ seed_of)
{
    const long long x = (long long)blockIdx.x * ORI_THREADS + threadIdx.x;
    if (x >= nt || !elig[x]) return;
    const uint32_t root = P[x] >> 1;
    if ((unsigned long long)__double_as_longlong(ori_dist2(xyz, x, seed.p)) == dkey[root]) atomicMin(&seed_of[root], (uint32_t)x);
}

// Launch: ORI_THREADS threads, ceil(nt / ORI_THREADS) workgroups.  seed_of: k_orient_seed's, or the labels (OA_SEED_KEEP).
// comp_flip[root] = parity of the seed ^ (the seed itself has to flip).  TOWARD: flip iff n . (p - v) < 0; AWAY: iff n . (v - p) < 0;
// fp64, (x x + y y) + z z, one rounding per operation; a dot of exactly 0 (or a NaN) keeps the sign.
__global__ __launch_bounds__(ORI_THREADS) void k_orient_sign(const uint32_t *__restrict__ P, const uint8_t *__restrict__ elig, const float *__restrict__ xyz,
                                                             const float *__restrict__ nrm, int nt, OrientSeed seed, const uint32_t *__restrict__ seed_of,
                                                             uint8_t *__restrict__ comp_flip, OrientInfo *__restrict__ info)
{
    const long long x = (long long)blockIdx.x * ORI_THREADS + threadIdx.x;
    const bool is_root = x < nt && elig[x] && (P[x] >> 1) == (uint32_t)x;
    ori_count(is_root, &info->n_components);
    if (!is_root) return;
    const uint32_t s = seed_of[x];
    if (s >= (uint32_t)nt) { comp_flip[x] = 0; return; }            // (never: a component has its root at least)
    uint32_t f = P[s] & 1u;
    if (seed.mode != 0) {
        double d[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = seed.mode == 1 ? __dsub_rn(seed.p[a], (double)xyz[3 * (long long)s + a]) : __dsub_rn((double)xyz[3 * (long long)s + a], seed.p[a]);
        const double dot = __dadd_rn(__dadd_rn(__dmul_rn((double)nrm[3 * (long long)s], d[0]), __dmul_rn((double)nrm[3 * (long long)s + 1], d[1])),
                                     __dmul_rn((double)nrm[3 * (long long)s + 2], d[2]));
        f ^= dot < 0.0 ? 1u : 0u;
    }
    comp_flip[x] = (uint8_t)f;
}

// Launch: ORI_THREADS threads, ceil(nt / ORI_THREADS) workgroups.  out may be nrm itself (a thread reads and writes its own row
// alone); out / flipped / component may be null.
__global__ __launch_bounds__(ORI_THREADS) void k_orient_apply(const uint32_t *__restrict__ P, const uint8_t *__restrict__ elig, const uint8_t *__restrict__ comp_flip,
                                                              const uint32_t *__restrict__ label, const float *nrm, int nt, float *out,
                                                              uint8_t *__restrict__ flipped, int32_t *__restrict__ component, OrientInfo *__restrict__ info)
{
    const long long x = (long long)blockIdx.x * ORI_THREADS + threadIdx.x;
    const bool in = x < nt;
    const bool ok = in && elig[x];
    uint32_t f = 0u, root = 0u;
    if (ok) { const uint32_t w = P[x]; root = w >> 1; f = (w & 1u) ^ comp_flip[root]; }
    ori_count(in && !ok, &info->n_left_out);
    ori_count(f != 0u, &info->n_flipped);
    if (!in) return;
    const uint32_t sign = f ? 0x80000000u : 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (out) out[3 * x + a] = __uint_as_float(__float_as_uint(nrm[3 * x + a]) ^ sign);
    if (flipped) flipped[x] = (uint8_t)f;
    if (component) component[x] = ok ? (int32_t)label[root] : -1;
}

#endif  // !OA_FAMILY_TU
#endif  // __HIPCC__
}  // namespace oa
