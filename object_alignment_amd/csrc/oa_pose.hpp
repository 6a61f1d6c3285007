// oa_pose.hpp -- many candidate poses against one target in one launch: the coarse stage in front of the (local) ICP loop.
//
// Every loop of this library follows the nearest correspondences from the current matrix_world; from a start that is far off it
// ends in the wrong pose.  The coarse stage (oa_coarse_align) scores a few hundred candidate poses by the truncated
// mean distance of a sample of the source to the target, refines the best few for some iterations and hands the cheapest to the
// loop.  A score is a COLD nearest-primitive query per (pose, sample point): what the 64-ary box tree (oa_bvh.hpp) is for.
//
//   k_pose_score<TRI, FULL>  one query = one (pose, sample point), one wave per query (bvh_wave_query<TRI>, no seed).  The pose's
//                            matrix takes the place of DevState::mx1 in co_find; the distance and its test are pair_eval's.  No
//                            normal-angle test, no weights.  A workgroup's queries belong to ONE pose; it writes one row:
//                              FULL = false   {K, sum dist, sum dist^2}                         (a score)
//                              FULL = true    the NSUMS sums of a point-metric step about `pivot` (a refinement step)
//   k_pose_rows_sum          rows -> per pose sums, fixed order
//   k_pose_solve             FULL rows -> sums -> the Kabsch solve -> pose <- pose @ float32(M), its inverse (one wave per pose)
//   k_centroid_rows          sum of the float32 m4_mul_v3 images of a point set, fp64, one row per workgroup
// Nothing here reads or writes DevState, keys, prev, win, wsafe or the history: a running loop does not see these launches.
#pragma once
#include "oa_bvh.hpp"

namespace oa {

constexpr int POSE_WPB = 4;          // waves (= queries in flight) per workgroup of k_pose_score
constexpr int POSE_NSCORE = 3;       // doubles per score row: K, sum dist, sum dist^2
constexpr int POSE_MAX_BPP = 4096;   // most workgroups (rows) per pose

// what every query of a launch shares: the base object's matrix and the call's own thresh and search radius
struct PoseBase {
    float  mx2[16], imx2[16];
    int32_t mx2_identity, pad;
    double thresh;
    double cut_a, cut_b;             // search_cutoff2's, derived from THIS call's thresh (+inf, 0: no radius)
    double pivot[3];                 // FULL: the sums are taken about it
};

struct Mat4f { float m[16]; };

#if defined(__HIPCC__)

// search_cutoff2's arithmetic on a radius that does not come from DevState
__device__ __forceinline__ float pose_cutoff2(double cut_a, double cut_b, float px, float py, float pz)
{
    if (!(cut_a < 1e300)) return INFINITY;
    const double pabs = fabs((double)px) + fabs((double)py) + fabs((double)pz);
    const double c = cut_a + cut_b * pabs;
    const double c2 = c * c * (1.0 + 1e-6);
    return c2 < 3.0e38 ? (float)c2 : INFINITY;
}

// Launch: 256 threads, n_poses x bpp workgroups; workgroup (pose, b) takes the sample points b * 4 + w, + bpp * 4, ... (w = wave).
// rows: n_poses x bpp rows of POSE_NSCORE / NSUMS doubles, every one written.
template <bool TRI, bool FULL>
__global__ __launch_bounds__(POSE_WPB * 64) void k_pose_score(PoseBase pb, const float *__restrict__ poses, const float *__restrict__ iposes,
                                                              const float4 *__restrict__ src4, const int *__restrict__ sample, int n_sample,
                                                              int bpp, BvhParams bp, const float4 *__restrict__ boxes,
                                                              const float4 *__restrict__ prims, const float4 *__restrict__ tri9,
                                                              double *__restrict__ rows)
{
    constexpr int W = FULL ? NSUMS : POSE_NSCORE;
    __shared__ float s_lb[POSE_WPB][BVH_MAX_LEVELS + 1][BVH_W];
    __shared__ unsigned long long s_mask[POSE_WPB][BVH_MAX_LEVELS + 1];
    __shared__ int s_node[POSE_WPB][BVH_MAX_LEVELS + 1];
    __shared__ double red[POSE_WPB][W];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const BvhLds lds{ &s_lb[w][0][0], BVH_W, &s_mask[w][0], 1, &s_node[w][0], 1 };
    const int pose = blockIdx.x / bpp, b = blockIdx.x - pose * bpp;                 // (workgroup-uniform)
    const float *__restrict__ mx1 = poses + 16ll * pose;
    const float *__restrict__ imx1 = FULL ? iposes + 16ll * pose : nullptr;
    // the wave's running sums: lane k owns number k (as k_bvh_search<TRI, true>)
    double lane_sum = 0.0;

    for (int s = b * POSE_WPB + w; s < n_sample; s += bpp * POSE_WPB) {
        const int i = sample[s];
        const float4 p4 = src4[i];
        float p[3];
        {   // co_find with the pose's matrix
            float wx, wy, wz;
            m4_mul_v3(mx1, p4.x, p4.y, p4.z, wx, wy, wz);
            if (pb.mx2_identity) { p[0] = wx; p[1] = wy; p[2] = wz; }
            else m4_mul_v3(pb.imx2, wx, wy, wz, p[0], p[1], p[2]);
        }
        float best = INFINITY, bx = 0.f, by = 0.f, bz = 0.f;
        uint32_t bidx = IDX_NONE;
        bvh_wave_query<TRI>(bp, boxes, prims, p, pose_cutoff2(pb.cut_a, pb.cut_b, p[0], p[1], p[2]), best, bidx, bx, by, bz, lds, lane);
        if (bidx == IDX_NONE) continue;                             // (wave-uniform)
        float qx = bx, qy = by, qz = bz;
        if (TRI) {
            float ta[3], tb[3], tc[3], rr[3];
            load_tri(tri9, bidx, ta, tb, tc);
            closest_on_tri(p, ta, tb, tc, rr);
            qx = rr[0]; qy = rr[1]; qz = rr[2];
        }
        // pair_eval's distance and test
        float ax = p[0], ay = p[1], az = p[2], wbx = qx, wby = qy, wbz = qz;
        if (!pb.mx2_identity) {
            m4_mul_v3(pb.mx2, p[0], p[1], p[2], ax, ay, az);
            m4_mul_v3(pb.mx2, qx, qy, qz, wbx, wby, wbz);
        }
        const double dist = v3_length(ax - wbx, ay - wby, az - wbz);
        if (!(dist < pb.thresh)) continue;
        double mine = 0.0;
#define OA_LANE_ADD(k, expr) mine = (lane == (k)) ? (expr) : mine
        if (FULL) {
            float vbx, vby, vbz;
            m4_mul_v3(imx1, wbx, wby, wbz, vbx, vby, vbz);          // imx1 @ (mx2 @ co1)
            const double a0 = (double)p4.x - pb.pivot[0], a1 = (double)p4.y - pb.pivot[1], a2 = (double)p4.z - pb.pivot[2];
            const double b0 = (double)vbx - pb.pivot[0], b1 = (double)vby - pb.pivot[1], b2 = (double)vbz - pb.pivot[2];
            OA_LANE_ADD(S_A, a0); OA_LANE_ADD(S_A + 1, a1); OA_LANE_ADD(S_A + 2, a2);
            OA_LANE_ADD(S_B, b0); OA_LANE_ADD(S_B + 1, b1); OA_LANE_ADD(S_B + 2, b2);
            OA_LANE_ADD(S_H + 0, b0 * a0); OA_LANE_ADD(S_H + 1, b0 * a1); OA_LANE_ADD(S_H + 2, b0 * a2);
            OA_LANE_ADD(S_H + 3, b1 * a0); OA_LANE_ADD(S_H + 4, b1 * a1); OA_LANE_ADD(S_H + 5, b1 * a2);
            OA_LANE_ADD(S_H + 6, b2 * a0); OA_LANE_ADD(S_H + 7, b2 * a1); OA_LANE_ADD(S_H + 8, b2 * a2);
            OA_LANE_ADD(S_AA, (a0 * a0 + a1 * a1) + a2 * a2);
            OA_LANE_ADD(S_BB, (b0 * b0 + b1 * b1) + b2 * b2);
            OA_LANE_ADD(S_K, 1.0);
            OA_LANE_ADD(S_D, dist);
            OA_LANE_ADD(S_DD, dist * dist);
        } else {
            OA_LANE_ADD(0, 1.0); OA_LANE_ADD(1, dist); OA_LANE_ADD(2, dist * dist);
        }
#undef OA_LANE_ADD
        lane_sum += mine;
    }
    // the waves' sums, added in order
    if (lane < W) red[w][lane] = lane_sum;
    __syncthreads();
    if (threadIdx.x < W) {
        double t = red[0][threadIdx.x];
        for (int k = 1; k < POSE_WPB; ++k) t += red[k][threadIdx.x];
        rows[(long long)blockIdx.x * W + threadIdx.x] = t;
    }
}

#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
// out[g * w + k] = rows[(g * per + 0) * w + k] + rows[(g * per + 1) * w + k] + ...: one workgroup of 64 threads per group g
__global__ __launch_bounds__(64) void k_pose_rows_sum(const double *__restrict__ rows, int per, int w, double *__restrict__ out)
{
    const int k = threadIdx.x;
    if (k >= w) return;
    const double *__restrict__ r = rows + (long long)blockIdx.x * per * w + k;
    double t = 0.0;
    for (int j = 0; j < per; ++j) t += r[(long long)j * w];
    out[(long long)blockIdx.x * w + k] = t;
}

// One refinement step of pose blockIdx.x: its FULL rows -> sums -> affine_matrix_from_points (rigid) -> matrix_world @ new_mat as
// the loop forms it (float32 new_mat, m4_mul_m4), and the inverse.  A pose with fewer than three pairs, or whose update is
// singular or not finite, stays as it is.
__global__ __launch_bounds__(64) void k_pose_solve(const double *__restrict__ rows, int bpp, double pvx, double pvy, double pvz,
                                                   float *__restrict__ poses, float *__restrict__ iposes)
{
    __shared__ double sums[NSUMS];
    const int k = threadIdx.x;
    if (k < NSUMS) {
        const double *__restrict__ r = rows + (long long)blockIdx.x * bpp * NSUMS + k;
        double t = 0.0;
        for (int j = 0; j < bpp; ++j) t += r[(long long)j * NSUMS];
        sums[k] = t;
    }
    __syncthreads();
    if (k != 0) return;
    double s[NSUMS], M[16];
    for (int j = 0; j < NSUMS; ++j) s[j] = sums[j];
    const double pv[3] = { pvx, pvy, pvz };
    if (!solve_from_sums(s, pv, false, M)) return;
    float *mx1 = poses + 16ll * blockIdx.x, *imx1 = iposes + 16ll * blockIdx.x;
    float cur[16], nm[16], mw[16], inv[16];
    for (int j = 0; j < 16; ++j) { cur[j] = mx1[j]; nm[j] = (float)M[j]; }
    m4_mul_m4(cur, nm, mw);
    bool finite = true;
    for (int j = 0; j < 16; ++j) finite = finite && fabsf(mw[j]) < INFINITY;
    if (!finite || !m4_inverted(mw, inv)) return;
    for (int j = 0; j < 16; ++j) finite = finite && fabsf(inv[j]) < INFINITY;
    if (!finite) return;
    for (int j = 0; j < 16; ++j) { mx1[j] = mw[j]; imx1[j] = inv[j]; }
}

// rows[blockIdx.x] = sum over the workgroup's points of M @ v (float32 m4_mul_v3, accumulated in fp64; points with a non-finite
// image are left out and not counted), {x, y, z, count}.  STRIDE = floats per point (3: packed xyz, 4: float4 slots).
// Launch: 256 threads, any number of workgroups (grid stride).
template <int STRIDE>
__global__ __launch_bounds__(256) void k_centroid_rows(const float *__restrict__ pts, int n, Mat4f mx, double *__restrict__ rows)
{
    __shared__ double red[4][4];
    double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float x, y, z;
        m4_mul_v3(mx.m, pts[STRIDE * i], pts[STRIDE * i + 1], pts[STRIDE * i + 2], x, y, z);
        if (fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY) {
            acc[0] += (double)x; acc[1] += (double)y; acc[2] += (double)z; acc[3] += 1.0;
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const double t = wave_sum(acc[k]); if (lane == 0) red[w][k] = t; }
    __syncthreads();
    if (threadIdx.x < 4) rows[4ll * blockIdx.x + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// sample[j] = the slot that holds the selection's point number j * stride in the caller's (vlist) order
__global__ __launch_bounds__(256) void k_pose_sample(const int *__restrict__ perm, int ns, int stride, int *__restrict__ sample)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= ns) return;
    const int pos = perm ? perm[s] : s;
    if (pos % stride == 0) sample[pos / stride] = s;
}
#endif  // !OA_FAMILY_TU

#endif  // __HIPCC__
}  // namespace oa
