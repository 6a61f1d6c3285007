// oa_recip.hpp -- reciprocal correspondences (EXTENSION, oa_set_reciprocal): keep a pair only if it is mutual.
//
// The contract (include/oa_icp.h):
//   Slot i holds a pair when pair_eval accepts it: dist < thresh, and the normal-angle test when it is on.  Let
//   b = imx1 @ (mx2 @ co1) be the float32 point that make_pairs emits in B (PairFetch::bx, by, bz, identical in vertex mode
//   and in surface mode), and p_k the selected source points: the packed src4 rows, i.e. the selection after vlist, stride and
//   sample_voxel.
//     - d2(b, p) = d2_metric(b, p), the project's fp32 difference form with its two fmas; symmetric in its arguments.
//     - m = min_k d2(b, p_k) over all selected slots.  A non-finite d2 never wins.
//     - The pair is kept iff d2(b, p_i) <= r2 * m, with r2 = (float)(ratio * ratio) and one fp32 multiply.
//     - With ratio = 1, the default, this reads "p_i is a nearest selected source point of its own correspondence".  Ties are
//       kept.  The result does not depend on index order.
//     - ratio lies in [1, 16]; anything else is OA_E_BAD_ARG.
//
// How: the source is rigid in its own frame, so ONE box tree over the selected source points, built once per oa_set_source
// in align-local space (build_bvh_arrays over src4, row stride 4; the primitive index in .w is the slot), serves every
// iteration at every pose.  k_recip_check walks it with bvh_wave_query<false> -- exact, and the (d2, index) every other search
// returns -- one wave per slot, seeded with the slot's own point: best = d2(b, p_i), bidx = i.  The seed bound is tight, so a
// settled pose descends to one or two leaves.  The verdict is one byte per slot; pair_fetch<.., RECIP = true> reads it
// (PairTest<true>::recip_ok, oa_kernels.hpp: a compile-time switch) and returns false for a slot whose byte is 0, after doing
// everything else it does.
#pragma once
#include "oa_bvh.hpp"

namespace oa {

constexpr int RECIP_WPB = 4;              // waves per workgroup of k_recip_check: one query each
constexpr int RECIP_FRAME_BLOCKS = 256;   // rows k_recip_frame leaves for the host
// the step's counters: rejected slots so far, workgroups that have finished, the last finished step's total (what the host reads)
constexpr int RECIP_COUNT_WORDS = 4;

#if defined(__HIPCC__)

// One wave per slot (workgroups loop when there are more slots than waves).  The pair is pair_fetch<false, METRIC_N>'s: the same
// pair, bit for bit, that the accumulation behind this launch will see; keys, prev and win are not written.  nrm is the plain
// NormalTest (RECIP = false: this kernel forms the verdict, it does not read one).  A slot without a pair is done (byte 1:
// nothing reads it).  Launched with ns >= 1 and count allocated (launch_recip skips an empty selection).  Rejected slots are
// counted with an integer atomic -- the total does not depend on the order -- and the last workgroup to finish moves the step's
// total to count[2] and clears the running words for the next step.
template <bool METRIC_N>
__global__ __launch_bounds__(RECIP_WPB * 64) void k_recip_check(const DevState *__restrict__ st, const float4 *__restrict__ src4, int ns,
                                                                const float *__restrict__ tgt_xyz,
                                                                const unsigned long long *__restrict__ keys,
                                                                const float4 *__restrict__ win, const float4 *__restrict__ tri9,
                                                                NormalTest nrm, const float *__restrict__ plane_tn, BvhParams bp,
                                                                const float4 *__restrict__ boxes, const float4 *__restrict__ prims,
                                                                float r2, unsigned char *__restrict__ recip_ok,
                                                                unsigned *__restrict__ count)
{
    if (st->halt) return;
    __shared__ float s_lb[RECIP_WPB][BVH_MAX_LEVELS + 1][BVH_W];
    __shared__ unsigned long long s_mask[RECIP_WPB][BVH_MAX_LEVELS + 1];
    __shared__ int s_node[RECIP_WPB][BVH_MAX_LEVELS + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const BvhLds lds{ &s_lb[w][0][0], BVH_W, &s_mask[w][0], 1, &s_node[w][0], 1 };
    const int n_waves = gridDim.x * RECIP_WPB;
    const double thresh = st->thresh;
    unsigned rejected = 0;                                          // wave-uniform

    for (int i = blockIdx.x * RECIP_WPB + w; i < ns; i += n_waves) {
        PairFetch f;
        bool keep = true;
        if (pair_fetch<false, METRIC_N>(st, src4, i, tgt_xyz, keys, nullptr, win, tri9, nrm, plane_tn, thresh, f)) {
            const float b[3] = { f.bx, f.by, f.bz };
            const float own = d2_metric(b[0], b[1], b[2], f.p.x, f.p.y, f.p.z);
            float best = INFINITY;
            uint32_t bidx = IDX_NONE;
            if (own < INFINITY) { best = own; bidx = (uint32_t)i; }
            float wx = f.p.x, wy = f.p.y, wz = f.p.z;               // (the winner's coordinates: not used)
            bvh_wave_query<false>(bp, boxes, prims, b, INFINITY, best, bidx, wx, wy, wz, lds, lane);
            keep = own <= r2 * best;
            if (!keep) ++rejected;
        }
        if (lane == 0) recip_ok[i] = keep ? 1 : 0;
    }
    if (lane == 0 && rejected) atomicAdd(&count[0], rejected);
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned done = atomicAdd(&count[1], 1u);
        if (done == gridDim.x - 1) {                                // the last workgroup: every other one's count is in
            __threadfence();
            count[2] = atomicExch(&count[0], 0u);
            atomicExch(&count[1], 0u);
        }
    }
}

#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
// the box of the finite coordinates of the packed source rows (float4 each): the Morton frame of the source tree.  One row
// {lo x, y, z, hi x, y, z} per workgroup; the host folds them (k_bbox_finite's shape, row stride 4)
__global__ __launch_bounds__(256) void k_recip_frame(const float4 *__restrict__ src4, int n, float *__restrict__ out /* blocks x 6 */)
{
    __shared__ float red[4][6];
    float b[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float4 p = src4[i];
        const float v[3] = { p.x, p.y, p.z };
        for (int a = 0; a < 3; ++a)
            if (fabsf(v[a]) < INFINITY) { b[a] = fminf(b[a], v[a]); b[3 + a] = fmaxf(b[3 + a], v[a]); }
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
        out[6 * blockIdx.x + a] = v;
    }
}
#endif  // !OA_FAMILY_TU

#endif  // __HIPCC__
}  // namespace oa
