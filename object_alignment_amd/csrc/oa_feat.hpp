// oa_feat.hpp -- coarse alignment from matched descriptors: nearest rows in descriptor space and candidate poses
// from triples of matched points.  The candidates go through the scoring and multi-start code of oa_pose.hpp.
//
//   k_fpfh<SECOND>         Fast Point Feature Histograms (Rusu, Blodow & Beetz 2009) of the target over the k-nearest lists of
//                          k_bvh_knn (a device buffer of nt x k indices), one lane per vertex, fp64.  SECOND = false: the SPFH
//                          table -- a lane counts its valid pairs per bin in LDS bytes (36 per lane: a run-time bin index never
//                          touches a register array), bin = count x (100 / m).  SECOND = true: FPFH = SPFH(p) + (1/m) sum over the
//                          valid pairs of SPFH(q) / l_q^2 in list order, every third scaled to 100, one rounding to float32.
//   k_match_features<DP>   for every row of fa the nearest and the second nearest row of fb (squared L2, fp32 vector ALU).  fb
//                          streams through a double-buffered LDS tile of FEAT_TB rows; a thread keeps FEAT_R query rows of DP
//                          floats in registers; every thread reads the same tile row at a time (an LDS broadcast).  The launch
//                          is (query blocks) x (splits of fb); a split writes its own (best key, second d2) per query and merges
//                          the best into the global key with atomicMin on (d2 bits << 32 | index): the lowest index wins ties.
//   k_match_finalize       per query: the winner's index and d2, and the second d2 = min over the splits of (the split's second
//                          if the split's best IS the global winner, else the split's best): independent of the split order.
//   k_triple_poses<WPB>    one wave per hypothesis (three matched pairs): the edge tests, the NSUMS row about a_0,
//                          solve_from_sums (rigid), float32(M @ mx_align) formed in fp64; a flag says whether it was accepted.
//   k_triple_compact       the accepted poses, in hypothesis order (one workgroup, an ordered scan; no atomics).
// Nothing here reads or writes DevState, keys, prev, win, wsafe or the history.
#pragma once
#include "oa_pose.hpp"                // (Mat4f; + oa_bvh.hpp, oa_kernels.hpp)

namespace oa {

constexpr int FPFH_BINS = 11, FPFH_DIM = 33;
constexpr int FPFH_THREADS = 256;
constexpr int FPFH_CNT_STRIDE = 36;  // LDS bytes per lane of the SPFH counters (9 dwords: odd, no bank conflicts between lanes)
constexpr int FEAT_TB = 64;          // rows of fb per LDS tile
constexpr int FEAT_R = 2;            // query rows per thread
constexpr int FEAT_THREADS = 256;
constexpr int FEAT_QPB = FEAT_THREADS * FEAT_R;   // queries per workgroup
constexpr int FEAT_MAX_DIM = 64;
constexpr int FEAT_MAX_SPLITS = 64;
constexpr unsigned long long FEAT_KEY_NONE = ~0ull;

// the padded row length a dim runs at (the pad columns are zero on both sides: they add +0 to every distance)
inline int feat_padded_dim(int dim) { return dim <= 8 ? 8 : dim <= 16 ? 16 : dim <= 36 ? 36 : 64; }

struct Mat4d { double m[16]; };

// The hashed draw of oa_feature_candidates, bit for bit (include/oa_icp.h states the same): all arithmetic in uint32, wrapping.
//   x = seed ^ (hyp * 0x9E3779B9) ^ ((slot + 1) * 0x85EBCA6B)
//   x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
//   index = (uint64(x) * n_pairs) >> 32
__host__ __device__ inline uint32_t feat_hash_index(uint32_t seed, uint32_t hyp, uint32_t slot, uint32_t n_pairs)
{
    uint32_t x = seed ^ (hyp * 0x9E3779B9u) ^ ((slot + 1u) * 0x85EBCA6Bu);
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return (uint32_t)(((unsigned long long)x * (unsigned long long)n_pairs) >> 32);
}

#if defined(__HIPCC__)

// The pair feature of vertex p (normal np) and neighbour q (normal nq), fp64: false when the pair is skipped (l = 0 or not finite,
// a normal that is zero or not finite, e parallel to n1).  bins: floor(11 (f1 + pi) / 2 pi), floor(11 (f2 + 1) / 2),
// floor(11 (f3 + 1) / 2), each clamped to 0 .. 10; l2 = |q - p|^2.
__host__ __device__ inline bool fpfh_pair(const double p[3], const double np[3], const double q[3], const double nq[3], int bins[3], double &l2,
                                          double coord[3])
{
    const double d0 = q[0] - p[0], d1 = q[1] - p[1], d2 = q[2] - p[2];
    l2 = (d0 * d0 + d1 * d1) + d2 * d2;
    const double l = sqrt(l2);
    if (!(l > 0.0) || !(l < INFINITY)) return false;
    const double npn = (np[0] * np[0] + np[1] * np[1]) + np[2] * np[2], nqn = (nq[0] * nq[0] + nq[1] * nq[1]) + nq[2] * nq[2];
    if (!(npn > 0.0) || !(npn < INFINITY) || !(nqn > 0.0) || !(nqn < INFINITY)) return false;
    double e[3] = { d0 / l, d1 / l, d2 / l };
    const double ap = (np[0] * e[0] + np[1] * e[1]) + np[2] * e[2], aq = (nq[0] * e[0] + nq[1] * e[1]) + nq[2] * e[2];
    const bool swap = fabs(ap) < fabs(aq);
    double n1[3], n2[3];
    for (int a = 0; a < 3; ++a) { n1[a] = swap ? nq[a] : np[a]; n2[a] = swap ? np[a] : nq[a]; e[a] = swap ? -e[a] : e[a]; }
    const double f3 = swap ? -aq : ap;                              // n1 . e
    double v[3] = { e[1] * n1[2] - e[2] * n1[1], e[2] * n1[0] - e[0] * n1[2], e[0] * n1[1] - e[1] * n1[0] };
    const double vl = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (!(vl > 0.0)) return false;
    for (int a = 0; a < 3; ++a) v[a] /= vl;
    const double w[3] = { n1[1] * v[2] - n1[2] * v[1], n1[2] * v[0] - n1[0] * v[2], n1[0] * v[1] - n1[1] * v[0] };
    const double f2 = (v[0] * n2[0] + v[1] * n2[1]) + v[2] * n2[2];
    const double f1 = atan2((w[0] * n2[0] + w[1] * n2[1]) + w[2] * n2[2], (n1[0] * n2[0] + n1[1] * n2[1]) + n1[2] * n2[2]);
    const double pi = 3.14159265358979323846;
    coord[0] = 11.0 * (f1 + pi) / (2.0 * pi); coord[1] = 11.0 * (f2 + 1.0) / 2.0; coord[2] = 11.0 * (f3 + 1.0) / 2.0;
    for (int a = 0; a < 3; ++a) bins[a] = (int)fmin(10.0, fmax(0.0, floor(coord[a])));
    return true;
}

// Launch: FPFH_THREADS threads, ceil(nt / FPFH_THREADS) workgroups; lane = vertex.  xyz, nrm: nt x 3 (the caller's order); idx: nt x k
// from k_bvh_knn (-1 = unfilled).  spfh: nt x 33 doubles (written when !SECOND, read when SECOND); out: nt x 33 floats (SECOND).
template <bool SECOND>
__global__ __launch_bounds__(FPFH_THREADS) void k_fpfh(const float *__restrict__ xyz, const float *__restrict__ nrm, const int32_t *__restrict__ idx,
                                                       int nt, int k, double *__restrict__ spfh, float *__restrict__ out)
{
    __shared__ unsigned char s_cnt[SECOND ? 4 : FPFH_THREADS * FPFH_CNT_STRIDE];
    const int i = blockIdx.x * FPFH_THREADS + threadIdx.x;
    if (i >= nt) return;                                            // (no barrier below: a lane's counters are its own)
    unsigned char *const cnt = SECOND ? nullptr : &s_cnt[threadIdx.x * FPFH_CNT_STRIDE];
    if (!SECOND)
        for (int b = 0; b < FPFH_DIM; ++b) cnt[b] = 0;
    const double p[3] = { (double)xyz[3ll * i], (double)xyz[3ll * i + 1], (double)xyz[3ll * i + 2] };
    const double np[3] = { (double)nrm[3ll * i], (double)nrm[3ll * i + 1], (double)nrm[3ll * i + 2] };
    double acc[FPFH_DIM];
#pragma unroll
    for (int b = 0; b < FPFH_DIM; ++b) acc[b] = 0.0;
    int m = 0;
    for (int j = 0; j < k; ++j) {
        const int qi = idx[(long long)i * k + j];
        if (qi < 0 || qi >= nt || qi == i) continue;
        const double q[3] = { (double)xyz[3ll * qi], (double)xyz[3ll * qi + 1], (double)xyz[3ll * qi + 2] };
        const double nq[3] = { (double)nrm[3ll * qi], (double)nrm[3ll * qi + 1], (double)nrm[3ll * qi + 2] };
        int bins[3];
        double l2, coord[3];
        if (!fpfh_pair(p, np, q, nq, bins, l2, coord)) continue;
        ++m;
        if (SECOND) {
            const double *__restrict__ row = spfh + (long long)qi * FPFH_DIM;
#pragma unroll
            for (int b = 0; b < FPFH_DIM; ++b) acc[b] += row[b] / l2;
        } else {
            cnt[bins[0]] += 1; cnt[FPFH_BINS + bins[1]] += 1; cnt[2 * FPFH_BINS + bins[2]] += 1;
        }
    }
    if (!SECOND) {
        const double unit = m > 0 ? 100.0 / (double)m : 0.0;
        for (int b = 0; b < FPFH_DIM; ++b) spfh[(long long)i * FPFH_DIM + b] = (double)cnt[b] * unit;
        return;
    }
    const double *__restrict__ own = spfh + (long long)i * FPFH_DIM;
#pragma unroll
    for (int b = 0; b < FPFH_DIM; ++b) acc[b] = m > 0 ? own[b] + acc[b] / (double)m : 0.0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        double sum = 0.0;
#pragma unroll
        for (int b = 0; b < FPFH_BINS; ++b) sum += acc[t * FPFH_BINS + b];
        const double scale = (sum > 0.0 && sum < INFINITY) ? 100.0 / sum : 0.0;
#pragma unroll
        for (int b = 0; b < FPFH_BINS; ++b) out[(long long)i * FPFH_DIM + t * FPFH_BINS + b] = (float)(acc[t * FPFH_BINS + b] * scale);
    }
}

// fa: na_pad x DP (na_pad a multiple of FEAT_QPB), fb: nb_pad x DP (nb_pad a multiple of FEAT_TB), both zero padded; bpen: nb_pad
// floats, 0 for a row that may answer and +inf for a zero row or a pad row.  Launch: FEAT_THREADS threads, (na_pad / FEAT_QPB,
// splits) workgroups; split s takes the tiles s * tps .. min(tiles, (s + 1) * tps) - 1.  part_key / part_second: splits x na_pad.
template <int DP>
__global__ __launch_bounds__(FEAT_THREADS) void k_match_features(const float *__restrict__ fa, const float *__restrict__ fb,
                                                                 const float *__restrict__ bpen, int na_pad, int tiles, int tps,
                                                                 unsigned long long *__restrict__ keys,
                                                                 unsigned long long *__restrict__ part_key, float *__restrict__ part_second)
{
    static_assert(DP % 4 == 0 && DP <= FEAT_MAX_DIM, "rows are read as float4");
    constexpr int V = DP / 4;                                  // float4 per row
    constexpr int TILE_V = FEAT_TB * V;                        // float4 per tile
    constexpr int LPT = (TILE_V + FEAT_THREADS - 1) / FEAT_THREADS;   // tile loads per thread
    __shared__ float4 s_b[2][TILE_V];
    __shared__ float s_pen[2][FEAT_TB];
    const int tid = threadIdx.x;
    const int split = blockIdx.y;
    const int t0 = split * tps, t1 = min(tiles, t0 + tps);     // (workgroup-uniform; t0 < t1 by the launch geometry)

    float a[FEAT_R][DP];
    int q[FEAT_R];
#pragma unroll
    for (int r = 0; r < FEAT_R; ++r) {
        q[r] = blockIdx.x * FEAT_QPB + r * FEAT_THREADS + tid;                     // < na_pad
        const float4 *__restrict__ row = reinterpret_cast<const float4 *>(fa + (size_t)q[r] * DP);
#pragma unroll
        for (int v = 0; v < V; ++v) { const float4 x = row[v]; a[r][4 * v] = x.x; a[r][4 * v + 1] = x.y; a[r][4 * v + 2] = x.z; a[r][4 * v + 3] = x.w; }
    }
    float best[FEAT_R], second[FEAT_R];
    int bidx[FEAT_R];
#pragma unroll
    for (int r = 0; r < FEAT_R; ++r) { best[r] = INFINITY; second[r] = INFINITY; bidx[r] = -1; }

    // a tile on its way: global -> registers (under the arithmetic of the tile before) -> LDS
    float4 stage[LPT];
    float stage_pen = 0.f;
#define OA_FEAT_LOAD_TILE(t)                                                                                            \
    {                                                                                                                   \
        const float4 *__restrict__ src_ = reinterpret_cast<const float4 *>(fb + (size_t)(t) * FEAT_TB * DP);            \
        _Pragma("unroll") for (int l = 0; l < LPT; ++l) {                                                               \
            const int e = l * FEAT_THREADS + tid;                                                                       \
            stage[l] = (l < LPT - 1 || TILE_V % FEAT_THREADS == 0 || e < TILE_V) ? src_[e < TILE_V ? e : 0] : float4{ 0.f, 0.f, 0.f, 0.f }; \
        }                                                                                                               \
        stage_pen = bpen[(size_t)(t) * FEAT_TB + (tid & (FEAT_TB - 1))];                                                \
    }
#define OA_FEAT_STORE_TILE(buf)                                                                                         \
    {                                                                                                                   \
        _Pragma("unroll") for (int l = 0; l < LPT; ++l) {                                                               \
            const int e = l * FEAT_THREADS + tid;                                                                       \
            if (l < LPT - 1 || TILE_V % FEAT_THREADS == 0 || e < TILE_V) s_b[buf][e] = stage[l];                        \
        }                                                                                                               \
        if (tid < FEAT_TB) s_pen[buf][tid] = stage_pen;                                                                 \
    }
    OA_FEAT_LOAD_TILE(t0)
    OA_FEAT_STORE_TILE(0)
    __syncthreads();
    int cur = 0;
    for (int t = t0; t < t1; ++t) {
        const bool more = t + 1 < t1;                           // (workgroup-uniform)
        if (more) OA_FEAT_LOAD_TILE(t + 1)                             // in flight under this tile's arithmetic
        const int j0 = t * FEAT_TB;
#pragma unroll 2
        for (int j = 0; j < FEAT_TB; ++j) {
            float acc[FEAT_R];
#pragma unroll
            for (int r = 0; r < FEAT_R; ++r) acc[r] = 0.f;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float4 b = s_b[cur][j * V + v];           // the same address in every lane: a broadcast
#pragma unroll
                for (int r = 0; r < FEAT_R; ++r) {
                    const float d0 = a[r][4 * v] - b.x, d1 = a[r][4 * v + 1] - b.y, d2 = a[r][4 * v + 2] - b.z, d3 = a[r][4 * v + 3] - b.w;
                    acc[r] += d0 * d0; acc[r] += d1 * d1; acc[r] += d2 * d2; acc[r] += d3 * d3;
                }
            }
            const float pen = s_pen[cur][j];
#pragma unroll
            for (int r = 0; r < FEAT_R; ++r) {
                const float d = acc[r] + pen;
                const bool lt = d < best[r];                    // ascending j: the lowest index keeps a tie
                second[r] = lt ? best[r] : fminf(second[r], d);
                bidx[r] = lt ? j0 + j : bidx[r];
                best[r] = lt ? d : best[r];
            }
        }
        if (more) OA_FEAT_STORE_TILE(cur ^ 1)                          // (the buffer the previous round read: every wave passed the barrier below since)
        __syncthreads();
        cur ^= 1;
    }
#pragma unroll
    for (int r = 0; r < FEAT_R; ++r) {
        const unsigned long long key = bidx[r] < 0 ? FEAT_KEY_NONE
                                                   : (((unsigned long long)__float_as_uint(best[r]) << 32) | (unsigned long long)(uint32_t)bidx[r]);
        part_key[(size_t)split * na_pad + q[r]] = key;
        part_second[(size_t)split * na_pad + q[r]] = second[r];
        if (key != FEAT_KEY_NONE) atomicMin(&keys[q[r]], key);
    }
#undef OA_FEAT_LOAD_TILE
#undef OA_FEAT_STORE_TILE
}

// a'_i = a_i - a_0, b'_i = b_i - a_0 (i = 0, 1, 2) -> the NSUMS row -> solve_from_sums about a_0.
// pair_s / pair_t: the kept pairs (source slot, target vertex); triples: n_hyp x 3 pair indices.  One wave per hypothesis, WPB
// hypotheses per workgroup.  poses: n_hyp x 16, flags: n_hyp (1 = accepted); both written for every hypothesis.
template <int WPB>
__global__ __launch_bounds__(WPB * 64) void k_triple_poses(const int *__restrict__ pair_s, const int *__restrict__ pair_t, int n_pairs,
                                                           const int *__restrict__ triples, int n_hyp, const float4 *__restrict__ src4,
                                                           const float *__restrict__ tgt_xyz, Mat4f mx1, Mat4f mx2, Mat4d mx_align,
                                                           double edge_tol, double min_edge, float *__restrict__ poses, int *__restrict__ flags)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int h = blockIdx.x * WPB + w;
    if (h >= n_hyp) return;                                        // (wave-uniform)
    // lanes 0 .. 2 fetch one pair each
    int pi = -1;
    float ax = 0.f, ay = 0.f, az = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
    if (lane < 3) {
        pi = triples[3ll * h + lane];
        if (pi >= 0 && pi < n_pairs) {
            const float4 p = src4[pair_s[pi]];
            const int t = pair_t[pi];
            m4_mul_v3(mx1.m, p.x, p.y, p.z, ax, ay, az);
            m4_mul_v3(mx2.m, tgt_xyz[3ll * t], tgt_xyz[3ll * t + 1], tgt_xyz[3ll * t + 2], bx, by, bz);
        } else pi = -1;
    }
    int id[3];
    double a[3][3], b[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        id[i] = __shfl(pi, i);
        a[i][0] = (double)__shfl(ax, i); a[i][1] = (double)__shfl(ay, i); a[i][2] = (double)__shfl(az, i);
        b[i][0] = (double)__shfl(bx, i); b[i][1] = (double)__shfl(by, i); b[i][2] = (double)__shfl(bz, i);
    }
    if (lane != 0) return;
    float *out = poses + 16ll * h;
    for (int e = 0; e < 16; ++e) out[e] = 0.f;
    flags[h] = 0;
    if (id[0] < 0 || id[1] < 0 || id[2] < 0 || id[0] == id[1] || id[0] == id[2] || id[1] == id[2]) return;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3;
        const double ea = sqrt(((a[i][0] - a[j][0]) * (a[i][0] - a[j][0]) + (a[i][1] - a[j][1]) * (a[i][1] - a[j][1])) + (a[i][2] - a[j][2]) * (a[i][2] - a[j][2]));
        const double eb = sqrt(((b[i][0] - b[j][0]) * (b[i][0] - b[j][0]) + (b[i][1] - b[j][1]) * (b[i][1] - b[j][1])) + (b[i][2] - b[j][2]) * (b[i][2] - b[j][2]));
        if (!(ea >= min_edge) || !(eb >= min_edge)) return;        // (also non-finite points)
        if (!(ea >= edge_tol * eb) || !(ea * edge_tol <= eb)) return;
    }
    double s[NSUMS];
    for (int k = 0; k < NSUMS; ++k) s[k] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a0 = a[i][0] - a[0][0], a1 = a[i][1] - a[0][1], a2 = a[i][2] - a[0][2];
        const double b0 = b[i][0] - a[0][0], b1 = b[i][1] - a[0][1], b2 = b[i][2] - a[0][2];
        s[S_A] += a0; s[S_A + 1] += a1; s[S_A + 2] += a2;
        s[S_B] += b0; s[S_B + 1] += b1; s[S_B + 2] += b2;
        s[S_H + 0] += b0 * a0; s[S_H + 1] += b0 * a1; s[S_H + 2] += b0 * a2;
        s[S_H + 3] += b1 * a0; s[S_H + 4] += b1 * a1; s[S_H + 5] += b1 * a2;
        s[S_H + 6] += b2 * a0; s[S_H + 7] += b2 * a1; s[S_H + 8] += b2 * a2;
        s[S_AA] += (a0 * a0 + a1 * a1) + a2 * a2;
        s[S_BB] += (b0 * b0 + b1 * b1) + b2 * b2;
        s[S_K] += 1.0;
    }
    double M[16];
    if (!solve_from_sums(s, a[0], false, M)) return;
    bool finite = true;
    float cand[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double t = 0.0;
            for (int k = 0; k < 4; ++k) t += M[4 * i + k] * mx_align.m[4 * k + j];
            cand[4 * i + j] = (float)t;
            finite = finite && fabsf(cand[4 * i + j]) < INFINITY;
        }
    float inv[16];
    if (!finite || !m4_inverted(cand, inv)) return;
    for (int e = 0; e < 16; ++e) out[e] = cand[e];
    flags[h] = 1;
}

#if !defined(OA_FAMILY_TU)      // plain kernels are compiled once, in the host translation unit (oa_icp.hip)
__global__ __launch_bounds__(256) void k_match_finalize(const unsigned long long *__restrict__ keys, const unsigned long long *__restrict__ part_key,
                                                        const float *__restrict__ part_second, int n, int na_pad, int splits,
                                                        int32_t *__restrict__ out_idx, float *__restrict__ out_d2, float *__restrict__ out_second)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long win = keys[i];
    if (win == FEAT_KEY_NONE) { out_idx[i] = -1; out_d2[i] = INFINITY; out_second[i] = INFINITY; return; }
    float sec = INFINITY;
    for (int s = 0; s < splits; ++s) {
        const unsigned long long k = part_key[(size_t)s * na_pad + i];
        const float cand = (k == win) ? part_second[(size_t)s * na_pad + i] : (k == FEAT_KEY_NONE ? INFINITY : __uint_as_float((uint32_t)(k >> 32)));
        sec = fminf(sec, cand);
    }
    out_idx[i] = (int32_t)(uint32_t)(win & 0xffffffffull);
    out_d2[i] = __uint_as_float((uint32_t)(win >> 32));
    out_second[i] = sec;
}

// out[rank of h among the accepted] = poses[h]; *n_out = how many.  Launch: ONE workgroup of 256 threads; thread t owns the
// hypotheses t * per .. (t + 1) * per - 1.
__global__ __launch_bounds__(256) void k_triple_compact(const float *__restrict__ poses, const int *__restrict__ flags, int n_hyp,
                                                        float *__restrict__ out, int *__restrict__ n_out)
{
    __shared__ int cnt[256];
    const int t = threadIdx.x;
    const int per = (n_hyp + 255) / 256;
    const int h0 = min(n_hyp, t * per), h1 = min(n_hyp, h0 + per);
    int mine = 0;
    for (int h = h0; h < h1; ++h) mine += flags[h] != 0;
    cnt[t] = mine;
    __syncthreads();
    if (t == 0) {                                                   // 256 additions: an exclusive scan in place
        int run = 0;
        for (int k = 0; k < 256; ++k) { const int c = cnt[k]; cnt[k] = run; run += c; }
        *n_out = run;
    }
    __syncthreads();
    int pos = cnt[t];
    for (int h = h0; h < h1; ++h)
        if (flags[h] != 0) {
            for (int e = 0; e < 16; ++e) out[16ll * pos + e] = poses[16ll * h + e];
            ++pos;
        }
}
#endif  // !OA_FAMILY_TU

#endif  // __HIPCC__
}  // namespace oa
