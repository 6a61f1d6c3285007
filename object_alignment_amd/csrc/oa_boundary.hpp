// oa_boundary.hpp -- the target's boundary (EXTENSION, oa_target_boundary / oa_set_reject_boundary): which mesh edges
// and vertices lie on the rim of an open mesh, which points of a cloud lie on its rim, and the rejection of a step's pairs whose
// correspondence lies there (Turk & Levoy 1994; Rusinkiewicz & Levoy 2001, 3.4).  Plain kernels, compiled once in the host
// translation unit (oa_icp.hip includes this file after oa_deviation.hpp).
//
// The contract (include/oa_icp.h):
//   MESH, integers only.  Local edge j of triangle t joins corners j and (j + 1) mod 3 (ab, bc, ca: FEAT_EDGE_AB/BC/CA's order).
//   An undirected edge {u, v}, u != v, is a boundary edge iff exactly one triangle -- each counted once -- lists both u and v.
//   u == v is never boundary; an edge of three or more triangles is not.  A vertex is a boundary vertex iff it ends a boundary
//   edge.  edge_mask[t] bit j = local edge j is boundary; vertex_mask[v] = 0 / 1.  Coordinates play no part.
//   CLOUD, the angle criterion (k, angle_deg), fp64 on the float32 values.  For vertex i with normal n: its neighbours are the
//   first k entries of its k-nearest row of k + 1 (k_bvh_knn) whose index is not i; u = normalise(n x e), v = n^ x u with e the
//   axis of n's smallest-magnitude component (lowest axis on ties); a neighbour whose projection (d.u, d.v) is (0, 0) or not
//   finite is skipped; theta = atan2(d.v, d.u), ascending; the gaps are the consecutive differences and the wrap-around gap
//   (theta_0 + 2 pi) - theta_last.  Flagged iff the largest gap > angle_deg pi / 180; also flagged: a zero or non-finite normal,
//   fewer than 3 usable neighbours.
//   A PAIR that pair_fetch accepts lies on the boundary iff -- surface mode -- closest_on_tri_region on the winning triangle
//   with the same co_find ends on an edge whose bit is set or on a vertex whose mask is 1 (a face: never); vertex mode: iff the
//   winning vertex is flagged.
//
//   k_mesh_boundary      one thread per (triangle, local edge) walks the lower vertex's corner row (k_pn_edge's walk) and counts
//                        the distinct triangles that hold the other end; the three threads of a triangle sit in one wave, so
//                        the edge byte is joined by two shuffles and stored by the first; both ends' vertex bytes are set to 1
//   k_cloud_boundary     one wave per vertex, lane j = entry j of its row; the order of the angles is never materialised:
//                        every lane finds its SUCCESSOR in the order (theta, lane) through lane broadcasts, its gap to it, and
//                        the wave takes the maximum
//   k_boundary_count     the set bits of a mask (integer atomics)
//   k_boundary_verdict   one thread per slot: byte 0 into the verdict bytes of the reciprocal check (oa_recip.hpp) for a pair on
//                        the boundary; nothing else is written
// No scratch, no floating-point atomics; every writer of a shared byte writes the same value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oa {

constexpr int BND_THREADS = 256;          // k_mesh_boundary (a multiple of 3 slots is not needed: see its wave layout), k_boundary_count
// k_boundary_verdict: large workgroups and few of them (two per CU, grid stride) -- every workgroup ends with two atomics on one
// line, and those serialise in L2 at some 12 ns each: 4 096 workgroups of 256 cost 100 us at 1M slots, 512 of 1 024 a tenth
constexpr int BND_VERDICT_THREADS = 1024;
constexpr int BND_EDGES_PER_WAVE = 63;    // k_mesh_boundary: 21 triangles x 3 edges per wave, lane 63 idles
constexpr int BND_WPB = 4;                // k_cloud_boundary: waves (vertices in flight) per workgroup
constexpr int BND_MAX_K = 63;             // k + 1 entries fit one wave
// the verdict's counters: rejected slots so far, workgroups that have finished, the last finished step's total (RECIP_COUNT_WORDS' layout)
constexpr int BND_COUNT_WORDS = 4;

#if defined(__HIPCC__) && !defined(OA_FAMILY_TU)

// Launch: BND_THREADS threads, ceil(n_tris / (21 * BND_THREADS / 64)) workgroups.  Lane l < 63 of a wave takes triangle
// 21 * wave + l / 3, local edge l % 3.  vertex_mask: zeroed by the caller.  (A triangle that lists the lower vertex twice is met
// twice in the row, at neighbouring positions -- the row is ascending by corner number -- and counted once.)
__global__ __launch_bounds__(BND_THREADS) void k_mesh_boundary(const int *__restrict__ tris, int n_tris, const int *__restrict__ order,
                                                               const long long *__restrict__ row_start, unsigned char *__restrict__ edge_mask,
                                                               unsigned char *__restrict__ vertex_mask)
{
    constexpr int TPW = BND_EDGES_PER_WAVE / 3;
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (BND_THREADS / 64) + (threadIdx.x >> 6);
    const long long t = wave * TPW + lane / 3;
    const int k = lane % 3;
    unsigned bit = 0u;
    if (lane < BND_EDGES_PER_WAVE && t < n_tris) {
        const int u = tris[3 * t + k], w = tris[3 * t + (k + 1) % 3];
        if (u != w) {
            const int lo = u < w ? u : w, hi = u < w ? w : u;
            int holders = 0;
            long long last = -1;
            for (long long j = row_start[lo]; j < row_start[lo + 1]; ++j) {
                const long long t2 = order[j] / 3;
                if (t2 == last) continue;
                last = t2;
                if (tris[3 * t2] == hi || tris[3 * t2 + 1] == hi || tris[3 * t2 + 2] == hi) ++holders;
            }
            if (holders == 1) {
                bit = 1u << k;
                vertex_mask[u] = 1; vertex_mask[w] = 1;
            }
        }
    }
    // (lanes 3 m, 3 m + 1, 3 m + 2 hold one triangle; every lane takes part in the shuffles)
    const unsigned b1 = (unsigned)__shfl_down((int)bit, 1, 64), b2 = (unsigned)__shfl_down((int)bit, 2, 64);
    if (lane < BND_EDGES_PER_WAVE && k == 0 && t < n_tris) edge_mask[t] = (unsigned char)(bit | b1 | b2);
}

// out[0] += the number of set bits among the low 3 bits of mask[0 .. n).  out: zeroed by the caller
__global__ __launch_bounds__(BND_THREADS) void k_boundary_count(const unsigned char *__restrict__ mask, long long n, unsigned *__restrict__ out)
{
    unsigned mine = 0u;
    for (long long i = (long long)blockIdx.x * BND_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * BND_THREADS)
        mine += (unsigned)__popc((unsigned)mask[i] & 7u);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) mine += (unsigned)__shfl_xor((int)mine, s, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(out, mine);
}

// Launch: 64 * BND_WPB threads, any number of workgroups (the vertices are dealt wave by wave, grid stride).  knn: nt rows of
// k + 1 indices (k_bvh_knn<false>: ascending (d2, index), -1 = unfilled), 3 <= k <= BND_MAX_K.  gap_min = angle_deg pi / 180.
__global__ __launch_bounds__(BND_WPB * 64) void k_cloud_boundary(const float *__restrict__ xyz, const float *__restrict__ normals,
                                                                 const int32_t *__restrict__ knn, int nt, int k, double gap_min,
                                                                 unsigned char *__restrict__ vertex_mask)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n_waves = gridDim.x * BND_WPB;
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    const double two_pi = 2.0 * 3.14159265358979323846;
    for (int i = blockIdx.x * BND_WPB + w; i < nt; i += n_waves) {              // (wave-uniform)
        const double nx = (double)normals[3ll * i], ny = (double)normals[3ll * i + 1], nz = (double)normals[3ll * i + 2];
        const double l2 = (nx * nx + ny * ny) + nz * nz;
        bool flagged = !(l2 > 0.0 && l2 < inf);
        if (!flagged) {
            const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
            const int axis = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
            const double ex = axis == 0 ? 1.0 : 0.0, ey = axis == 1 ? 1.0 : 0.0, ez = axis == 2 ? 1.0 : 0.0;
            double ux = ny * ez - nz * ey, uy = nz * ex - nx * ez, uz = nx * ey - ny * ex;
            const double ul = sqrt((ux * ux + uy * uy) + uz * uz), nl = sqrt(l2);
            ux /= ul; uy /= ul; uz /= ul;
            const double hx = nx / nl, hy = ny / nl, hz = nz / nl;
            const double vx = hy * uz - hz * uy, vy = hz * ux - hx * uz, vz = hx * uy - hy * ux;
            // the row: the first k entries that are not i
            const int32_t e = lane <= k ? knn[(long long)i * (k + 1) + lane] : (int32_t)i;
            const bool other = lane <= k && e != (int32_t)i;
            const unsigned long long others = __ballot(other);
            const int pos = __popcll(others & ((1ull << lane) - 1ull));
            double theta = inf;
            if (other && pos < k && e >= 0) {
                const double dx = (double)xyz[3ll * e] - (double)xyz[3ll * i], dy = (double)xyz[3ll * e + 1] - (double)xyz[3ll * i + 1],
                             dz = (double)xyz[3ll * e + 2] - (double)xyz[3ll * i + 2];
                const double a = (dx * ux + dy * uy) + dz * uz, b = (dx * vx + dy * vy) + dz * vz;
                const bool finite = fabs(a) < inf && fabs(b) < inf;
                if (finite && !(a == 0.0 && b == 0.0)) theta = atan2(b, a);
            }
            const bool usable = theta < inf;
            const int n_usable = __popcll(__ballot(usable));
            if (n_usable < 3) flagged = true;
            else {
                // the successor of (theta, lane) in the ascending order with ties by lane, and the smallest angle of all
                double next = inf, first = inf;
                for (int m = 0; m <= k; ++m) {
                    const double tm = __shfl(theta, m, 64);
                    first = tm < first ? tm : first;
                    const bool after = tm > theta || (tm == theta && m > lane);
                    if (after && tm < next) next = tm;
                }
                double gap = 0.0;
                if (usable) gap = next < inf ? next - theta : (first + two_pi) - theta;
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) { const double g2 = __shfl_xor(gap, s, 64); gap = g2 > gap ? g2 : gap; }
                flagged = gap > gap_min;
            }
        }
        if (lane == 0) vertex_mask[i] = flagged ? 1 : 0;
    }
}

// One thread per slot (grid stride).  The pair is pair_fetch<false, false>'s -- keys, prev and win are not written -- with the
// plain NormalTest.  A slot without a pair, or whose byte is already 0 (k_recip_check), is done.  tris / edge_mask: surface mode.
// Rejected slots are counted per workgroup and added with one integer atomic each; the last workgroup to finish moves the step's total to count[2] and clears the
// running words for the next step (k_recip_check's protocol).  Launched with ns >= 1.
__global__ __launch_bounds__(BND_VERDICT_THREADS) void k_boundary_verdict(const DevState *__restrict__ st, const float4 *__restrict__ src4, int ns,
                                                                  const float *__restrict__ tgt_xyz, const unsigned long long *__restrict__ keys,
                                                                  const float4 *__restrict__ win, const float4 *__restrict__ tri9, NormalTest nrm,
                                                                  const int *__restrict__ tris, const unsigned char *__restrict__ edge_mask,
                                                                  const unsigned char *__restrict__ vertex_mask, unsigned char *__restrict__ verdict,
                                                                  unsigned *__restrict__ count)
{
    if (st->halt) return;
    const double thresh = st->thresh;
    unsigned rejected = 0u;
    for (long long base = (long long)blockIdx.x * BND_VERDICT_THREADS; base < ns; base += (long long)gridDim.x * BND_VERDICT_THREADS) {
        const int i = (int)(base + threadIdx.x);
        bool on_rim = false;
        if (i < ns && verdict[i] != 0) {
            PairFetch f;
            if (pair_fetch<false, false>(st, src4, i, tgt_xyz, keys, nullptr, win, tri9, nrm, nullptr, thresh, f)) {
                if (tri9) {
                    float cf[3], ta[3], tb[3], tc[3], r[3];
                    co_find(st, f.p.x, f.p.y, f.p.z, cf[0], cf[1], cf[2]);
                    load_tri(tri9, f.idx, ta, tb, tc);
                    const int feature = closest_on_tri_region(cf, ta, tb, tc, r);
                    if (feature >= FEAT_VERT_A) on_rim = vertex_mask[tris[3ll * f.idx + (feature - FEAT_VERT_A)]] != 0;
                    else if (feature >= FEAT_EDGE_AB) on_rim = (((unsigned)edge_mask[f.idx] >> (feature - FEAT_EDGE_AB)) & 1u) != 0u;
                } else on_rim = vertex_mask[f.idx] != 0;
            }
            if (on_rim) verdict[i] = 0;
        }
        rejected += (unsigned)__popcll(__ballot(on_rim));               // (wave-uniform)
    }
    __shared__ unsigned s_rejected[BND_VERDICT_THREADS / 64];
    if ((threadIdx.x & 63) == 0) s_rejected[threadIdx.x >> 6] = rejected;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0u;
        for (int w = 0; w < BND_VERDICT_THREADS / 64; ++w) total += s_rejected[w];
        if (total) atomicAdd(&count[0], total);                     // (one atomic per workgroup)
        __threadfence();
        const unsigned done = atomicAdd(&count[1], 1u);
        if (done == gridDim.x - 1) {                                // the last workgroup: every other one's count is in
            __threadfence();
            count[2] = atomicExch(&count[0], 0u);
            atomicExch(&count[1], 0u);
        }
    }
}

#endif  // __HIPCC__ && !OA_FAMILY_TU
}  // namespace oa
