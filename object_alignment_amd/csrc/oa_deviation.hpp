// oa_deviation.hpp -- the deviation report (oa_deviation): per selected source point the correspondence at the
// current pose, the world-space pair distance the accumulation kernels see, its SIGN against the target, and fit statistics.
// Plain kernels, compiled once in the host translation unit (oa_icp.hip includes this file after oa_sort.hpp).
//
//   closest_on_tri_region   closest_on_tri (oa_kernels.hpp) + where on the triangle the point lies; the same float32 operations
//                           in the same order, the same r
//   k_pn_face               per triangle: unit face normal n_t and the three corner angles (fp64 on the float32 vertices)
//   k_pn_row_start          per vertex: where its corners start in the stable order of the 3 n_tris corners by vertex index
//   k_pn_vertex             per vertex: N_v = sum angle n_t over its corners, in ascending (triangle, corner) order
//   k_pn_edge               per (triangle, local edge): N_e = sum n_t' over ALL triangles with the undirected edge, ascending t'
//   k_deviation             per slot: pair_fetch<false, false> (the accumulation kernels' pair), region, pseudo-normal, sign, the
//                           outputs in the caller's order, the select key, the LDS histogram, one row of partials per workgroup
//   k_dev_finish            the rows, in a fixed order -> DevResult
//   k_dev_select_hist/_scan the radix select of oa_set_robust_auto (k_select_hist / k_select_scan) over the keys, one quantile per
//                           blockIdx.y / workgroup, with a state of its own instead of DevState's
//
// THE SIGN.  The nearest triangle's face normal names the wrong side wherever the closest point lies on an edge or a vertex of a
// non-convex (or merely sharp) mesh.  The angle-weighted pseudo-normal (Baerentzen & Aanaes 2005) does not: with p = co_find,
// r = co1 and N the pseudo-normal of the feature r lies on (face: n_t; edge: the sum of its faces' n_t; vertex: the sum of its
// corners' angle n_t), s = ((p - r)_x N_x + (p - r)_y N_y) + (p - r)_z N_z in fp64 is negative exactly inside.
// Everything is summed in an order that depends on the mesh alone; no floating-point atomics: two builds give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oa {

// feature codes of closest_on_tri_region (oa_deviation's `feature` output)
constexpr int FEAT_FACE = 0, FEAT_EDGE_AB = 1, FEAT_EDGE_BC = 2, FEAT_EDGE_CA = 3, FEAT_VERT_A = 4, FEAT_VERT_B = 5, FEAT_VERT_C = 6;

// closest_on_tri with the region it ended in.  A COPY of that function's arithmetic (it and its callers stay as they are):
// every float32 operation below is one of its operations on its operands, in its order -- tools/region_check.hip compares
// the two bit for bit.
__host__ __device__ inline int closest_on_tri_region(const float *p, const float *a, const float *b, const float *c, float *r)
{
    const float ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2], cx = c[0], cy = c[1], cz = c[2];
    const float px = p[0], py = p[1], pz = p[2];
    const float abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
    const float apx = px - ax, apy = py - ay, apz = pz - az, bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const float cpx = px - cx, cpy = py - cy, cpz = pz - cz, cbx = cx - bx, cby = cy - by, cbz = cz - bz;
#define OA_DOT3(ux, uy, uz, vx, vy, vz) (((ux) * (vx) + (uy) * (vy)) + (uz) * (vz))
    const float d1 = OA_DOT3(abx, aby, abz, apx, apy, apz), d2 = OA_DOT3(acx, acy, acz, apx, apy, apz);
    const float d3 = OA_DOT3(abx, aby, abz, bpx, bpy, bpz), d4 = OA_DOT3(acx, acy, acz, bpx, bpy, bpz);
    const float d5 = OA_DOT3(abx, aby, abz, cpx, cpy, cpz), d6 = OA_DOT3(acx, acy, acz, cpx, cpy, cpz);
#undef OA_DOT3
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float d43 = d4 - d3, d56 = d5 - d6;
    const bool at_a = d1 <= 0.0f && d2 <= 0.0f;
    const bool at_b = d3 >= 0.0f && d4 <= d3;
    const bool on_ab = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
    const bool at_c = d6 >= 0.0f && d5 <= d6;
    const bool on_ac = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
    const bool on_bc = va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f;
    enum { AT_A, AT_B, ON_AB, AT_C, ON_AC, ON_BC, INSIDE };
    const int region = at_a ? AT_A : at_b ? AT_B : on_ab ? ON_AB : at_c ? AT_C : on_ac ? ON_AC : on_bc ? ON_BC : INSIDE;
    const float num = region == ON_AB ? d1 : region == ON_AC ? d2 : region == ON_BC ? d43 : 1.0f;
    const float den = region == ON_AB ? d1 - d3 : region == ON_AC ? d2 - d6 : region == ON_BC ? d43 + d56 : (va + vb) + vc;
    const float q = num / den;
    const float s1 = region == INSIDE ? vb * q : q;
    const float s2 = vc * q;
    const bool from_b = region == ON_BC || region == AT_B, from_c = region == AT_C;
    const bool vertex = region == AT_A || region == AT_B || region == AT_C, inside = region == INSIDE;
    const bool along_ac = region == ON_AC, along_cb = region == ON_BC;
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
    return region == AT_A ? FEAT_VERT_A : region == AT_B ? FEAT_VERT_B : region == AT_C ? FEAT_VERT_C
         : region == ON_AB ? FEAT_EDGE_AB : region == ON_BC ? FEAT_EDGE_BC : region == ON_AC ? FEAT_EDGE_CA : FEAT_FACE;
}

constexpr int DEV_THREADS = 256;          // k_deviation: one thread per slot
constexpr int DEV_MAX_BINS = 1024;        // histogram bins (+ one underflow and one overflow bin)
constexpr int DEV_MAX_Q = 8;              // quantiles per call
constexpr int DEV_FIN_THREADS = 256;      // k_dev_finish

// what the signed distance takes its sign from
constexpr int DEV_SIGN_NONE = 0, DEV_SIGN_MESH = 1, DEV_SIGN_VERTEX = 2;

struct DevHist {                          // bins over [lo, hi) of signed_d: bin = floor((d - lo) scale), scale = n_bins / (hi - lo)
    double lo, hi, scale;
    int32_t n_bins, pad;
};

// one row per workgroup of k_deviation, and (row 0 of `result`) the call's totals
struct DevRow {
    double sum_d, sum_dd, sum_signed;     // over the inliers (dist < thresh)
    long long n_valid, n_inlier, n_inside, n_unsigned;
    unsigned long long max_bits;          // the bits of the largest dist among the valid slots (non-negative doubles order as integers) ...
    long long max_index;                  // ... and the lowest caller-order position that attains it (-1: no valid slot)
};

struct DevSelect {                        // the state of one quantile's radix select, between its launches
    double p, q;                          // the quantile asked for; the order statistic found
    uint32_t prefix, rank, kq;
    uint32_t k_min;                       // the smallest 1-based rank the select may land on (oa_set_trim: 3); 0 = no floor
};

struct DevOut {                           // per-slot outputs, caller order; each may be nullptr
    long long *idx;
    float *closest;
    double *dist, *signed_d;
    signed char *feature;
};

#if defined(__HIPCC__) && !defined(OA_FAMILY_TU)

__device__ __forceinline__ bool pn_usable(double x, double y, double z)
{
    const double l2 = (x * x + y * y) + z * z;
    return l2 > 0.0 && l2 < (double)INFINITY;
}

__device__ __forceinline__ double pn_angle(const double u[3], const double v[3])
{
    const double cx = u[1] * v[2] - u[2] * v[1], cy = u[2] * v[0] - u[0] * v[2], cz = u[0] * v[1] - u[1] * v[0];
    return atan2(sqrt((cx * cx + cy * cy) + cz * cz), (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]);
}

// face_n: n_tris x 3 doubles, the unit normal cross(b - a, c - a) (1 / sqrt((x x + y y) + z z)); angle: n_tris x 3, the corner
// angles atan2(|u x v|, u . v).  A triangle whose cross product has zero or non-finite squared length gets zeros: it then adds
// nothing to any sum
__global__ __launch_bounds__(256) void k_pn_face(const float *__restrict__ xyz, const int *__restrict__ tris, int n_tris,
                                                 double *__restrict__ face_n, double *__restrict__ angle)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tris) return;
    double v[3][3];
    for (int k = 0; k < 3; ++k) {
        const long long i = tris[3 * t + k];
        for (int a = 0; a < 3; ++a) v[k][a] = (double)xyz[3 * i + a];
    }
    double e[3][3];                                                  // e[k] = v[k+1] - v[k]
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) e[k][a] = v[(k + 1) % 3][a] - v[k][a];
    const double u[3] = { e[0][0], e[0][1], e[0][2] };               // b - a
    const double w[3] = { -e[2][0], -e[2][1], -e[2][2] };            // c - a
    const double nx = u[1] * w[2] - u[2] * w[1], ny = u[2] * w[0] - u[0] * w[2], nz = u[0] * w[1] - u[1] * w[0];
    const bool ok = pn_usable(nx, ny, nz);
    const double inv = ok ? 1.0 / sqrt((nx * nx + ny * ny) + nz * nz) : 0.0;
    face_n[3 * t] = ok ? nx * inv : 0.0; face_n[3 * t + 1] = ok ? ny * inv : 0.0; face_n[3 * t + 2] = ok ? nz * inv : 0.0;
    for (int k = 0; k < 3; ++k) {                                    // corner k: between v[k+1] - v[k] and v[k+2] - v[k]
        const double p[3] = { e[k][0], e[k][1], e[k][2] };
        const double q[3] = { -e[(k + 2) % 3][0], -e[(k + 2) % 3][1], -e[(k + 2) % 3][2] };
        angle[3 * t + k] = ok ? pn_angle(p, q) : 0.0;
    }
}

// row_start[v] = first position in `order` (the stable order of the corners by vertex index) of a corner at a vertex >= v;
// row_start[n_verts] = n_corners.  One binary search per vertex: nothing assumes a valence
__global__ __launch_bounds__(256) void k_pn_row_start(const int *__restrict__ tris, const int *__restrict__ order, long long n_corners, int n_verts,
                                                      long long *__restrict__ row_start)
{
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v > n_verts) return;
    long long lo = 0, hi = n_corners;                                // corners [0, lo) are at vertices < v, [hi, n) at vertices >= v
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if ((long long)tris[order[mid]] < v) lo = mid + 1; else hi = mid;
    }
    row_start[v] = lo;
}

// one thread per vertex: its row is stable, hence ascending by corner number 3 t + k, i.e. by (triangle, corner)
__global__ __launch_bounds__(256) void k_pn_vertex(const int *__restrict__ order, const long long *__restrict__ row_start, int n_verts,
                                                   const double *__restrict__ face_n, const double *__restrict__ angle, float *__restrict__ vertex_n)
{
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_verts) return;
    double s[3] = { 0.0, 0.0, 0.0 };
    for (long long j = row_start[v]; j < row_start[v + 1]; ++j) {
        const long long c = order[j], t = c / 3;
        const double w = angle[c];
        for (int a = 0; a < 3; ++a) s[a] += w * face_n[3 * t + a];
    }
    for (int a = 0; a < 3; ++a) vertex_n[3 * v + a] = (float)s[a];
}

// one thread per (triangle, local edge): edge k joins corners k and k + 1 (ab, bc, ca).  The row of the edge's lower vertex
// lists every triangle that holds it, ascending; those that also have the edge add their n_t.  (A triangle that lists the
// lower vertex twice is met twice -- it has no area and adds zeros.)
__global__ __launch_bounds__(256) void k_pn_edge(const int *__restrict__ tris, int n_tris, const int *__restrict__ order,
                                                 const long long *__restrict__ row_start, const double *__restrict__ face_n, float *__restrict__ edge_n)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= 3ll * n_tris) return;
    const long long t = e / 3;
    const int k = (int)(e - 3 * t);
    const int u = tris[3 * t + k], w = tris[3 * t + (k + 1) % 3];
    const int lo = u < w ? u : w, hi = u < w ? w : u;
    double s[3] = { 0.0, 0.0, 0.0 };
    for (long long j = row_start[lo]; j < row_start[lo + 1]; ++j) {
        const long long t2 = order[j] / 3;
        const int i0 = tris[3 * t2], i1 = tris[3 * t2 + 1], i2 = tris[3 * t2 + 2];
        const bool has = (min(i0, i1) == lo && max(i0, i1) == hi) || (min(i1, i2) == lo && max(i1, i2) == hi) || (min(i2, i0) == lo && max(i2, i0) == hi);
        if (has)
            for (int a = 0; a < 3; ++a) s[a] += face_n[3 * t2 + a];
    }
    for (int a = 0; a < 3; ++a) edge_n[3 * e + a] = (float)s[a];
}

// lexicographic (largest dist bits, lowest index): does not depend on the order of the merges
__device__ __forceinline__ void dev_max_merge(unsigned long long &bits, long long &index, unsigned long long b2, long long i2)
{
    if (i2 >= 0 && (index < 0 || b2 > bits || (b2 == bits && i2 < index))) { bits = b2; index = i2; }
}

// Launch: DEV_THREADS threads, ceil(ns_pad / DEV_THREADS) workgroups (slots >= ns only have their keys reset).  Leaves every
// key KEY_EMPTY for the next search, as k_decode_keys does.  rows: one DevRow per workgroup; dkeys: ns select keys (the bits of
// (float)dist; RKEY_NONE without a correspondence); hist: n_bins + 2 counts, zeroed by the caller, or nullptr.
__global__ __launch_bounds__(DEV_THREADS) void k_deviation(const DevState *__restrict__ st, const float4 *__restrict__ src4, int ns, int ns_pad,
                                                           const float *__restrict__ tgt_xyz, unsigned long long *keys,
                                                           const float4 *__restrict__ win, const float4 *__restrict__ tri9, double thresh,
                                                           int sign_mode, const int *__restrict__ tris, const double *__restrict__ face_n,
                                                           const float *__restrict__ vertex_n, const float *__restrict__ edge_n,
                                                           const float *__restrict__ tgt_n, const int *__restrict__ perm, DevOut out,
                                                           uint32_t *__restrict__ dkeys, DevHist hg, unsigned long long *__restrict__ hist,
                                                           DevRow *__restrict__ rows)
{
    __shared__ unsigned int bins[DEV_MAX_BINS + 2];
    __shared__ double red_d[DEV_THREADS / 64][3];
    __shared__ long long red_n[DEV_THREADS / 64][4];
    __shared__ unsigned long long red_b[DEV_THREADS / 64];
    __shared__ long long red_i[DEV_THREADS / 64];
    const int i = blockIdx.x * DEV_THREADS + threadIdx.x;
    const bool with_hist = hist != nullptr && hg.n_bins > 0;
    if (with_hist) {
        for (int b = threadIdx.x; b < hg.n_bins + 2; b += DEV_THREADS) bins[b] = 0u;
        __syncthreads();
    }
    double sum_d = 0.0, sum_dd = 0.0, sum_s = 0.0;
    long long cnt[4] = { 0, 0, 0, 0 };                               // valid, inlier, inside, unsigned
    unsigned long long max_bits = 0ull;
    long long max_index = -1;
    if (i < ns) {
        PairFetch f;
        const NormalTest no_test{ nullptr, nullptr, 0.0 };
        const bool inlier = pair_fetch<false, false>(st, src4, i, tgt_xyz, (const unsigned long long *)keys, nullptr, win, tri9, no_test, nullptr, thresh, f);
        const long long o = perm ? perm[i] : i;
        const bool valid = f.idx != IDX_NONE;
        const double nan = __longlong_as_double(0x7FF8000000000000ll);
        float r[3] = { __int_as_float(0x7FC00000), __int_as_float(0x7FC00000), __int_as_float(0x7FC00000) };
        double dist = nan, sd = nan;
        int feature = -1;
        if (valid) {
            // co_find and co1 once more, through pair_fetch's own functions on its operands: the same bits
            float cf[3];
            co_find(st, f.p.x, f.p.y, f.p.z, cf[0], cf[1], cf[2]);
            double n[3] = { 0.0, 0.0, 0.0 };
            if (tri9) {
                float ta[3], tb[3], tc[3];
                load_tri(tri9, f.idx, ta, tb, tc);
                feature = closest_on_tri_region(cf, ta, tb, tc, r);
                if (sign_mode == DEV_SIGN_MESH) {
                    if (feature == FEAT_FACE) {
                        for (int a = 0; a < 3; ++a) n[a] = face_n[3ll * f.idx + a];
                    } else if (feature <= FEAT_EDGE_CA) {
                        for (int a = 0; a < 3; ++a) n[a] = (double)edge_n[9ll * f.idx + 3 * (feature - FEAT_EDGE_AB) + a];
                    } else {
                        const long long v = tris[3ll * f.idx + (feature - FEAT_VERT_A)];
                        for (int a = 0; a < 3; ++a) n[a] = (double)vertex_n[3 * v + a];
                    }
                }
            } else {
                for (int a = 0; a < 3; ++a) r[a] = tgt_xyz[3ll * f.idx + a];
                if (sign_mode == DEV_SIGN_VERTEX)
                    for (int a = 0; a < 3; ++a) n[a] = (double)tgt_n[3ll * f.idx + a];
            }
            dist = f.dist;
            sd = dist;
            cnt[0] = 1;
            if (sign_mode != DEV_SIGN_NONE) {
                if (pn_usable(n[0], n[1], n[2])) {
                    const double dx = (double)cf[0] - (double)r[0], dy = (double)cf[1] - (double)r[1], dz = (double)cf[2] - (double)r[2];
                    const double s = (dx * n[0] + dy * n[1]) + dz * n[2];
                    if (s < 0.0) sd = -dist;
                } else cnt[3] = 1;
            }
            if (sd < 0.0) cnt[2] = 1;
            if (inlier) { cnt[1] = 1; sum_d = dist; sum_dd = dist * dist; sum_s = sd; }
            max_bits = (unsigned long long)__double_as_longlong(dist);
            max_index = o;
            if (with_hist) {
                int b;
                if (sd < hg.lo) b = 0;
                else if (!(sd < hg.hi)) b = hg.n_bins + 1;
                else {
                    const double fb = floor((sd - hg.lo) * hg.scale);
                    b = 1 + (fb < (double)(hg.n_bins - 1) ? (int)fb : hg.n_bins - 1);
                }
                atomicAdd(&bins[b], 1u);                                 // (integer counts: the order of the atomics is immaterial)
            }
        }
        if (out.idx) out.idx[o] = valid ? (long long)f.idx : -1ll;
        if (out.closest) { out.closest[3 * o] = r[0]; out.closest[3 * o + 1] = r[1]; out.closest[3 * o + 2] = r[2]; }
        if (out.dist) out.dist[o] = dist;
        if (out.signed_d) out.signed_d[o] = sd;
        if (out.feature) out.feature[o] = (signed char)feature;
        dkeys[i] = valid ? (uint32_t)__float_as_int((float)dist) : RKEY_NONE;
    }
    if (i < ns_pad) keys[i] = KEY_EMPTY;
    // the workgroup's row: a butterfly over the wave, then the waves in order (a fixed pattern: the same bits on every run)
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        sum_d += __shfl_xor(sum_d, s, 64); sum_dd += __shfl_xor(sum_dd, s, 64); sum_s += __shfl_xor(sum_s, s, 64);
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt[k] += __shfl_xor(cnt[k], s, 64);
        const unsigned long long b2 = __shfl_xor(max_bits, s, 64);
        const long long i2 = __shfl_xor(max_index, s, 64);
        dev_max_merge(max_bits, max_index, b2, i2);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red_d[wave][0] = sum_d; red_d[wave][1] = sum_dd; red_d[wave][2] = sum_s;
        for (int k = 0; k < 4; ++k) red_n[wave][k] = cnt[k];
        red_b[wave] = max_bits; red_i[wave] = max_index;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        DevRow row;
        double d[3] = { red_d[0][0], red_d[0][1], red_d[0][2] };
        long long n[4] = { red_n[0][0], red_n[0][1], red_n[0][2], red_n[0][3] };
        unsigned long long mb = red_b[0];
        long long mi = red_i[0];
        for (int w = 1; w < DEV_THREADS / 64; ++w) {
            for (int k = 0; k < 3; ++k) d[k] += red_d[w][k];
            for (int k = 0; k < 4; ++k) n[k] += red_n[w][k];
            dev_max_merge(mb, mi, red_b[w], red_i[w]);
        }
        row.sum_d = d[0]; row.sum_dd = d[1]; row.sum_signed = d[2];
        row.n_valid = n[0]; row.n_inlier = n[1]; row.n_inside = n[2]; row.n_unsigned = n[3];
        row.max_bits = mb; row.max_index = mi;
        rows[blockIdx.x] = row;
    }
    if (with_hist) {
        for (int b = threadIdx.x; b < hg.n_bins + 2; b += DEV_THREADS) {
            const unsigned int v = bins[b];
            if (v) atomicAdd(&hist[b], (unsigned long long)v);
        }
    }
}

// One workgroup: thread t adds rows t, t + DEV_FIN_THREADS, ... in ascending order, then the threads' sums are joined by a
// fixed tree in LDS (stride 128, 64, ... 1).  result: one DevRow
__global__ __launch_bounds__(DEV_FIN_THREADS) void k_dev_finish(const DevRow *__restrict__ rows, int n_rows, DevRow *__restrict__ result)
{
    __shared__ DevRow red[DEV_FIN_THREADS];
    DevRow a;
    a.sum_d = a.sum_dd = a.sum_signed = 0.0;
    a.n_valid = a.n_inlier = a.n_inside = a.n_unsigned = 0;
    a.max_bits = 0ull; a.max_index = -1;
    for (int r = threadIdx.x; r < n_rows; r += DEV_FIN_THREADS) {
        const DevRow b = rows[r];
        a.sum_d += b.sum_d; a.sum_dd += b.sum_dd; a.sum_signed += b.sum_signed;
        a.n_valid += b.n_valid; a.n_inlier += b.n_inlier; a.n_inside += b.n_inside; a.n_unsigned += b.n_unsigned;
        dev_max_merge(a.max_bits, a.max_index, b.max_bits, b.max_index);
    }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = DEV_FIN_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            DevRow &x = red[threadIdx.x];
            const DevRow &y = red[threadIdx.x + s];
            x.sum_d += y.sum_d; x.sum_dd += y.sum_dd; x.sum_signed += y.sum_signed;
            x.n_valid += y.n_valid; x.n_inlier += y.n_inlier; x.n_inside += y.n_inside; x.n_unsigned += y.n_unsigned;
            dev_max_merge(x.max_bits, x.max_index, y.max_bits, y.max_index);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *result = red[0];
}

// ---- the quantiles: oa_set_robust_auto's radix select (sel_digit / sel_above / sel_count / sel_clear / sel_flush and the walk
// of k_select_scan), with the state in DevSelect -- one per quantile -- instead of DevState.  hist: n_q x SEL_LEVELS x SEL_BINS
// counts, zeroed by the caller.  Grid of k_dev_select_hist: (blocks, n_q); of k_dev_select_scan: n_q workgroups.
__global__ __launch_bounds__(SEL_THREADS) void k_dev_select_hist(const DevSelect *__restrict__ sel, const uint32_t *__restrict__ dkeys, int ns, int level,
                                                                 uint32_t *__restrict__ hist)
{
    __shared__ uint32_t bins[SEL_BINS];
    const DevSelect s = sel[blockIdx.y];
    if (level > 0 && s.kq == 0u) return;
    sel_clear(bins);
    for (long long base = (long long)blockIdx.x * blockDim.x; base < ns; base += (long long)gridDim.x * blockDim.x) {
        const long long i = base + threadIdx.x;
        const uint32_t key = i < ns ? dkeys[i] : RKEY_NONE;
        sel_count(bins, key != RKEY_NONE && (level == 0 || sel_above(key, level) == s.prefix), sel_digit(key, level));
    }
    sel_flush(bins, hist + ((long long)blockIdx.y * SEL_LEVELS + level) * SEL_BINS);
}

__global__ __launch_bounds__(SEL_THREADS) void k_dev_select_scan(DevSelect *__restrict__ sel, const uint32_t *__restrict__ hist, int level)
{
    constexpr int PER = SEL_BINS / SEL_THREADS;
    __shared__ uint32_t wave_tot[SEL_THREADS / 64];
    DevSelect *st = sel + blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t *h = hist + ((long long)blockIdx.x * SEL_LEVELS + level) * SEL_BINS;
    uint32_t cnt[PER], mine = 0u;
#pragma unroll
    for (int k = 0; k < PER; ++k) { cnt[k] = h[threadIdx.x * PER + k]; mine += cnt[k]; }
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine, total = 0u;
    for (int w = 0; w < SEL_THREADS / 64; ++w) { if (w < wave) before += wave_tot[w]; total += wave_tot[w]; }
    uint32_t rank = st->rank, prefix = st->prefix, kq = st->kq;
    if (level == 0) {
        kq = total;
        prefix = 0u;
        double k = ceil(st->p * (double)kq);                        // the rule of oa_set_robust_auto: the ceil(p K)-th smallest, 1-based
        k = k < 1.0 ? 1.0 : (k > (double)kq ? (double)kq : k);
        rank = (uint32_t)k - 1u;
        const uint32_t floor_k = st->k_min < kq ? st->k_min : kq;   // (k_min = 0, the quantiles: rank stays what it was)
        if (floor_k > 0u && rank < floor_k - 1u) rank = floor_k - 1u;
    }
    __syncthreads();                                                // (every thread has read the state before one of them writes it)
    if (kq != 0u && rank >= before && rank - before < mine) {       // exactly one thread
        uint32_t r = rank - before, bin = threadIdx.x * PER;
        bool found = false;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (!found && r < cnt[k]) found = true;
            if (!found) { r -= cnt[k]; ++bin; }
        }
        prefix = level == 2 ? (prefix << 10) | bin : (prefix << 11) | bin;
        st->prefix = prefix;
        st->rank = r;
        if (level == 0) st->kq = kq;
        if (level == SEL_LEVELS - 1) st->q = (double)__uint_as_float(prefix);
    }
    if (kq == 0u && threadIdx.x == 0 && level == 0) { st->kq = 0u; st->prefix = 0u; st->rank = 0u; st->q = __longlong_as_double(0x7FF8000000000000ll); }
}

#endif  // __HIPCC__ && !OA_FAMILY_TU
}  // namespace oa
