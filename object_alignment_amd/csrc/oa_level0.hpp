// oa_level0.hpp -- level 0 of k_nn_search_sorted as the kernel runs it: the fold of one block of sorted vertices into "can this lane's
// point (or point pair) rule the whole block out?".  The four kinds of level 0 (sorted_level0, oa_kernels.hpp) differ only in
// where a trip's tile rows come from and which gap function they call (oa_pairgap.hpp, oa_quadgap.hpp, oa_octgap.hpp: the gaps,
// their images and the proofs of their bounds).  All carry the same chain, level0_chain: the block's minimum gap in {m, odd},
// grown by v_min3_f32 alone (two comparisons per instruction; v_min_f32, v_min3_f32 and v_cmp_*_f32 issue at half v_sub_f32's
// rate on gfx950), and end in one compare against the threshold per block.  Here: the chain, and the trips and the verdict of
// the two kinds that fold pairs of the lane's points; the two per-point kinds' trips are written out in the kernel, on the chain.
// A fold function is ONE TRIP -- 16 vertices, or four images; its caller unrolls the block's trips around it and asks for the
// verdict:
//     float m[..], odd[..];
//     for (c = 0 .. trips) level0_xxx<R>(rows of trip c, c == 0, ..., m, odd);         (#pragma unroll)
//     any = level0_pair_hits<R>(m, odd, qthr, hit);                                    (per point: a compare against thr1[r])
// (The loop stays with the caller on purpose: the compiler optimises a function before it inlines it, and a whole block folded
//  inside one came back with all its tile reads ahead of all its arithmetic -- <2, 64, false> at 800 B of scratch.  For the same
//  reason the per-point kinds' trips and verdict stay in the kernel: as functions they cost scratch, or the fold's schedule.)
// Kept apart from the kernel so that tools/valu_rates.hip times these very functions.
#pragma once

#include <hip/hip_runtime.h>
#include "oa_pairgap.hpp"
#include "oa_quadgap.hpp"
#include "oa_octgap.hpp"

namespace oa {

// N gaps (N even) into the chain {m, odd}.  first: the block's first trip, nothing carried in.  Each min3 takes the chain's
// value and two gaps; the gap left over is carried in odd and joins the next trip's first min3.
template <int N>
__device__ __forceinline__ void level0_chain(const float (&a)[N], bool first, float &m, float &odd)
{
    static_assert(N >= 2 && N % 2 == 0, "level0_chain: pairs of gaps");
    float v = first ? a[0] : __builtin_fminf(__builtin_fminf(m, odd), a[0]);
#pragma unroll
    for (int k = 1; k + 1 < N; k += 2) v = __builtin_fminf(__builtin_fminf(v, a[k]), a[k + 1]);   // v_min3_f32
    m = v;
    odd = a[N - 1];
}

// Vertex pairs x point pairs: the same pair images, quad_gap against the lane's point pairs {qhm, qhw} (signed: no modifier on
// the min's sources).  Per 16 vertices and point pair 24 subtracts and 4 min3.
template <int R>
__device__ __forceinline__ void level0_point_pairs(const float4 *mw, bool first, const float (&qhm)[R / 2], const float (&qhw)[R / 2],
                                                   float (&qm)[R / 2], float (&qodd)[R / 2])
{
    float4 MW[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) MW[k] = mw[k];
#pragma unroll
    for (int p = 0; p < R / 2; ++p) {
        float a[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            a[2 * k] = quad_gap(MW[k].x, MW[k].y, qhm[p], qhw[p]); a[2 * k + 1] = quad_gap(MW[k].z, MW[k].w, qhm[p], qhw[p]);
        }
        level0_chain(a, first, qm[p], qodd[p]);
    }
}

// Images x point pairs: four images {mm, ww, ws} (img: three float4 -- their four mm, their four ww, their four ws), oct_gap
// against the point pairs {qhm, qhw' = max(hw, c)}.  Three tile reads, 16 subtracts and 2 min3 per point pair, however many
// sorted positions an image stands for.
template <int R>
__device__ __forceinline__ void level0_images(const float4 *img, bool first, const float (&qhm)[R / 2], const float (&qhw)[R / 2],
                                              float (&qm)[R / 2], float (&qodd)[R / 2])
{
    const float4 MM = img[0], WW = img[1], WS = img[2];
#pragma unroll
    for (int p = 0; p < R / 2; ++p) {
        const float a[4] = { oct_gap(MM.x, WW.x, WS.x, qhm[p], qhw[p]), oct_gap(MM.y, WW.y, WS.y, qhm[p], qhw[p]),
                             oct_gap(MM.z, WW.z, WS.z, qhm[p], qhw[p]), oct_gap(MM.w, WW.w, WS.w, qhm[p], qhw[p]) };
        level0_chain(a, first, qm[p], qodd[p]);
    }
}

// The block's verdict per point PAIR (2p, 2p + 1): a hit unless the minimum is above the pair's threshold (a NaN is a hit); returns
// whether any pair hit.  A pair that cannot rule the block out marks BOTH its points; level 0v and levels 1-3
// decide per point (a hit the per-point fold would not have given is wasted work there, never a wrong answer.  Folding the
// block again per point for exactly the per-point hit[r] measured slower: 17.17 against 16.03 ms per step at 1M <-> 1M,
// profiles/r13a_point_pairs.txt).
template <int R>
__device__ __forceinline__ bool level0_pair_hits(const float (&qm)[R / 2], const float (&qodd)[R / 2], const float (&qthr)[R / 2], bool (&hit)[R])
{
    bool any = false;
#pragma unroll
    for (int p = 0; p < R / 2; ++p) {
        hit[2 * p] = hit[2 * p + 1] = !(__builtin_fminf(qm[p], qodd[p]) > qthr[p]);
        any |= hit[2 * p];
    }
    return any;
}

}  // namespace oa
