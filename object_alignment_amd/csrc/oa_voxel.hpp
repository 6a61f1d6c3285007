// oa_voxel.hpp -- voxel-grid downsampling (oa_voxel_downsample): one output row per occupied cell of a uniform
// grid -- the members' mean, their number, the member nearest to the mean (the "representative") and the normalised sum of
// their normals.  Plain kernels, compiled once in the host translation unit (oa_icp.hip includes this file after oa_sort.hpp).
//
//   k_voxel_bbox         per workgroup {min xyz, max xyz} and the number of points whose three coordinates are finite
//   k_voxel_keys         key = (c_z dims_y + c_y) dims_x + c_x, c = floor(((double)x - o) / voxel); all ones when not finite
//   k_voxel_key_part     a <= 32-bit slice of the keys: one key of the lexicographic order (oa_sort.hpp, lex_order_next)
//   k_voxel_heads        1 where the sorted key changes
//   k_voxel_row_start    first sorted position of every row (+ the end of the last)
//   k_voxel_row_chunks   chunks a LONG row (more than VOX_CHUNK members) is cut into; 0 for a short one
//   k_voxel_reduce       short rows: one group of VOX_GROUP lanes per row.  Writes count, mean, normal
//   k_voxel_reduce_long  long rows: one wave per chunk of VOX_CHUNK members -> partial sums
//   k_voxel_finish_long  long rows: the partials added in chunk order -> mean, normal
//   k_voxel_rep, k_voxel_rep_long, k_voxel_rep_finish_long   the same three shapes for the arg-min of (d2, index)
//
// THE ORDER OF SUMMATION (a function of the input alone: of the row's length L and the stable sorted order m_0 < m_1 < ...
// of its members' indices).  Every sum is fp64, starts at +0 and has no fused multiply-add and no atomics.
//   L <= VOX_CHUNK:  lane j of the row's 8 lanes adds m_j, m_{j+8}, m_{j+16}, ... in ascending order; the 8 lane sums s_0 .. s_7
//                    are then joined by a fixed butterfly: t_j = s_j + s_{j^4}; u_j = t_j + t_{j^2}; sum = u_0 + u_1, i.e.
//                    ((s_0 + s_4) + (s_2 + s_6)) + ((s_1 + s_5) + (s_3 + s_7)).
//   L >  VOX_CHUNK:  the row is cut into chunks of VOX_CHUNK consecutive members (the last one shorter).  In a chunk, lane l
//                    of 64 adds members l, l + 64, ... in ascending order, and the 64 lane sums are joined by the butterfly
//                    with strides 32, 16, 8, 4, 2, 1 (stride 32 first).  The chunks' sums are added in chunk order.
// The arg-min merges (d2, index) pairs lexicographically, which does not depend on any order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oa {

constexpr int VOX_CHUNK = 512;          // members per chunk of a long row (a fixed constant: part of the summation order)
constexpr int VOX_GROUP = 8;            // lanes per short row
constexpr int VOX_THREADS = 256;
constexpr int VOX_BBOX_BLOCKS = 256;
constexpr int VOX_MAX_DIM = 1 << 21;

// most chunks the long rows of n points can have: a long row of L > VOX_CHUNK members has ceil(L / VOX_CHUNK) <= L / VOX_CHUNK + 1
// chunks and there are fewer than n / VOX_CHUNK long rows
inline size_t voxel_max_chunks(size_t n) { return 2 * (n / VOX_CHUNK) + 2; }

#if defined(__HIPCC__)

struct VoxelGrid {
    double o[3];        // origin
    double h;           // cell edge
    long long dx, dy;   // dims_x, dims_y
};

__device__ __forceinline__ bool vox_finite3(float x, float y, float z)
{
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}

// Launch: VOX_THREADS threads, any number of workgroups.  A workgroup that saw no finite point writes +inf / -inf and 0.
__global__ __launch_bounds__(VOX_THREADS) void k_voxel_bbox(const float *__restrict__ xyz, int n, float *__restrict__ out /* blocks x 6 */,
                                                            int *__restrict__ out_count /* blocks */)
{
    __shared__ float red[VOX_THREADS / 64][6];
    __shared__ int cnt[VOX_THREADS / 64];
    float b[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    int count = 0;
    for (long long i = (long long)blockIdx.x * VOX_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * VOX_THREADS) {
        const float v[3] = { xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2] };
        if (vox_finite3(v[0], v[1], v[2])) {
            ++count;
            for (int a = 0; a < 3; ++a) { b[a] = fminf(b[a], v[a]); b[3 + a] = fmaxf(b[3 + a], v[a]); }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            b[a] = fminf(b[a], __shfl_xor(b[a], o, 64));
            b[3 + a] = fmaxf(b[3 + a], __shfl_xor(b[3 + a], o, 64));
        }
        count += __shfl_xor(count, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 6; ++a) red[threadIdx.x >> 6][a] = b[a];
        cnt[threadIdx.x >> 6] = count;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        float v = red[0][a];
        for (int k = 1; k < VOX_THREADS / 64; ++k) v = a < 3 ? fminf(v, red[k][a]) : fmaxf(v, red[k][a]);
        out[blockIdx.x * 6 + a] = v;
    }
    if (threadIdx.x == 6) {
        int s = 0;
        for (int k = 0; k < VOX_THREADS / 64; ++k) s += cnt[k];
        out_count[blockIdx.x] = s;
    }
}

// the cell of one coordinate: three exactly defined fp64 operations (a true division: the unit is built without fast-math
// and with -ffp-contract=off)
__device__ __forceinline__ long long vox_cell(float x, double o, double h) { return (long long)floor(((double)x - o) / h); }

__global__ __launch_bounds__(VOX_THREADS) void k_voxel_keys(const float *__restrict__ xyz, int n, VoxelGrid g, unsigned long long *__restrict__ keys)
{
    const long long i = (long long)blockIdx.x * VOX_THREADS + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    unsigned long long k = ~0ull;
    if (vox_finite3(x, y, z)) {
        const long long cx = vox_cell(x, g.o[0], g.h), cy = vox_cell(y, g.o[1], g.h), cz = vox_cell(z, g.o[2], g.h);
        k = (unsigned long long)((cz * g.dy + cy) * g.dx + cx);
    }
    keys[i] = k;
}

// out[j] = bits [shift, shift + width) of the key of the point at position j of `order` (order == nullptr: of point j)
__global__ __launch_bounds__(VOX_THREADS) void k_voxel_key_part(const unsigned long long *__restrict__ keys, int n, int shift, unsigned mask,
                                                                uint32_t *__restrict__ out)
{
    const long long j = (long long)blockIdx.x * VOX_THREADS + threadIdx.x;
    if (j >= n) return;
    out[j] = (uint32_t)(keys[j] >> shift) & mask;
}

__global__ __launch_bounds__(VOX_THREADS) void k_voxel_heads(const unsigned long long *__restrict__ keys, const int *__restrict__ order, int n_finite,
                                                             int *__restrict__ head)
{
    const long long j = (long long)blockIdx.x * VOX_THREADS + threadIdx.x;
    if (j >= n_finite) return;
    head[j] = (j == 0 || keys[order[j]] != keys[order[j - 1]]) ? 1 : 0;
}

// off = the exclusive scan of head (off[n_finite] = the number of rows): the point at sorted position j is in row
// off[j] + head[j] - 1
__global__ __launch_bounds__(VOX_THREADS) void k_voxel_row_start(const int *__restrict__ head, const long long *__restrict__ off, int n_finite,
                                                                 int *__restrict__ row_start /* rows + 1 */)
{
    const long long j = (long long)blockIdx.x * VOX_THREADS + threadIdx.x;
    if (j >= n_finite) return;
    if (head[j]) row_start[off[j]] = (int)j;
    if (j == 0) row_start[off[n_finite]] = n_finite;
}

__global__ __launch_bounds__(VOX_THREADS) void k_voxel_row_chunks(const int *__restrict__ row_start, int n_rows, int *__restrict__ n_chunks)
{
    const long long r = (long long)blockIdx.x * VOX_THREADS + threadIdx.x;
    if (r >= n_rows) return;
    const int len = row_start[r + 1] - row_start[r];
    n_chunks[r] = len > VOX_CHUNK ? (len + VOX_CHUNK - 1) / VOX_CHUNK : 0;
}

// the row's mean (one fp64 division by the count, one rounding) and its normal (the project's rule: n * (1 / sqrt((x x + y y) + z z)),
// fp64, rounded once; the zero row for a sum of zero or non-finite length)
__device__ __forceinline__ void vox_write_row(const double s[6], int count, long long row, bool with_normals, float *__restrict__ out_xyz,
                                              float *__restrict__ out_nrm)
{
    const double c = (double)count;
    for (int a = 0; a < 3; ++a) out_xyz[3 * row + a] = (float)(s[a] / c);
    if (with_normals) {
        const double l2 = (s[3] * s[3] + s[4] * s[4]) + s[5] * s[5];
        const bool ok = l2 > 0.0 && l2 < (double)INFINITY;
        const double inv = ok ? 1.0 / sqrt(l2) : 0.0;
        for (int a = 0; a < 3; ++a) out_nrm[3 * row + a] = ok ? (float)(s[3 + a] * inv) : 0.0f;
    }
}

// members first, first + STEP, ... below `end` of the sorted order, added in ascending order into s; four gathers in flight
template <int STEP>
__device__ __forceinline__ void vox_sum_members(const float *__restrict__ xyz, const float *__restrict__ nrm, const int *__restrict__ order, int first,
                                                int end, double s[6])
{
    for (int m = first; m < end; m += 4 * STEP) {
        int idx[4];
        float v[4][6];
#pragma unroll
        for (int u = 0; u < 4; ++u) idx[u] = m + u * STEP < end ? order[m + u * STEP] : -1;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                v[u][a] = idx[u] >= 0 ? xyz[3 * (long long)idx[u] + a] : 0.0f;
                v[u][3 + a] = (idx[u] >= 0 && nrm) ? nrm[3 * (long long)idx[u] + a] : 0.0f;
            }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (idx[u] >= 0)
#pragma unroll
                for (int a = 0; a < 6; ++a) s[a] += (double)v[u][a];
    }
}

// Launch: VOX_THREADS threads, ceil(n_rows * VOX_GROUP / VOX_THREADS) workgroups.  Every row gets its count; long rows get
// their mean from k_voxel_finish_long.
__global__ __launch_bounds__(VOX_THREADS) void k_voxel_reduce(const float *__restrict__ xyz, const float *__restrict__ nrm, const int *__restrict__ order,
                                                              const int *__restrict__ row_start, int n_rows, float *__restrict__ out_xyz,
                                                              float *__restrict__ out_nrm, int *__restrict__ out_count, int *__restrict__ max_members)
{
    const long long row = ((long long)blockIdx.x * VOX_THREADS + threadIdx.x) / VOX_GROUP;
    const int j = threadIdx.x & (VOX_GROUP - 1);
    const bool live = row < n_rows;
    int b = 0, e = 0;
    if (live) { b = row_start[row]; e = row_start[row + 1]; }
    const int len = e - b;
    double s[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    if (len <= VOX_CHUNK) vox_sum_members<VOX_GROUP>(xyz, nrm, order, b + j, e, s);
#pragma unroll
    for (int o = VOX_GROUP / 2; o > 0; o >>= 1)
#pragma unroll
        for (int a = 0; a < 6; ++a) s[a] += __shfl_xor(s[a], o, 64);
    int mx = len;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(max_members, mx);        // (an integer maximum: the order is immaterial)
    if (live && j == 0) {
        out_count[row] = len;
        if (len <= VOX_CHUNK) vox_write_row(s, len, row, nrm != nullptr, out_xyz, out_nrm);
    }
}

// the row of chunk w: the last r with chunk_off[r] <= w (rows without chunks repeat their successor's offset and are never it)
__device__ __forceinline__ int vox_row_of_chunk(const long long *__restrict__ chunk_off, int n_rows, long long w)
{
    int lo = 0, hi = n_rows;                                         // chunk_off[lo] <= w < chunk_off[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (chunk_off[mid] <= w) lo = mid; else hi = mid;
    }
    return lo;
}

// Launch: VOX_THREADS threads, any number of workgroups: the waves walk the chunks with a stride.  partial: chunks x 6.
__global__ __launch_bounds__(VOX_THREADS) void k_voxel_reduce_long(const float *__restrict__ xyz, const float *__restrict__ nrm, const int *__restrict__ order,
                                                                   const int *__restrict__ row_start, const long long *__restrict__ chunk_off, int n_rows,
                                                                   double *__restrict__ partial)
{
    const int lane = threadIdx.x & 63;
    const long long total = chunk_off[n_rows], n_waves = (long long)gridDim.x * (VOX_THREADS / 64);
    for (long long w = (long long)blockIdx.x * (VOX_THREADS / 64) + (threadIdx.x >> 6); w < total; w += n_waves) {
        const int r = vox_row_of_chunk(chunk_off, n_rows, w);
        const long long b = (long long)row_start[r] + (w - chunk_off[r]) * VOX_CHUNK;
        const int e = (int)min(b + VOX_CHUNK, (long long)row_start[r + 1]);
        double s[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        vox_sum_members<64>(xyz, nrm, order, (int)b + lane, e, s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int a = 0; a < 6; ++a) s[a] += __shfl_xor(s[a], o, 64);
        if (lane == 0)
            for (int a = 0; a < 6; ++a) partial[6 * w + a] = s[a];
    }
}

__global__ __launch_bounds__(VOX_THREADS) void k_voxel_finish_long(const int *__restrict__ row_start, const long long *__restrict__ chunk_off, int n_rows,
                                                                   const double *__restrict__ partial, bool with_normals, float *__restrict__ out_xyz,
                                                                   float *__restrict__ out_nrm)
{
    const long long r = (long long)blockIdx.x * VOX_THREADS + threadIdx.x;
    if (r >= n_rows) return;
    const long long c0 = chunk_off[r], c1 = chunk_off[r + 1];
    if (c1 == c0) return;
    double s[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (long long c = c0; c < c1; ++c)
        for (int a = 0; a < 6; ++a) s[a] += partial[6 * c + a];
    vox_write_row(s, row_start[r + 1] - row_start[r], r, with_normals, out_xyz, out_nrm);
}

// ---- the representative: arg-min of (d2, index), d2 = (dx dx + dy dy) + dz dz in fp64 against the row's FLOAT32 mean -----------
struct VoxBest { double d2; int idx; };

__device__ __forceinline__ void vox_best_merge(VoxBest &a, double d2, int idx)
{
    if (idx >= 0 && (a.idx < 0 || d2 < a.d2 || (d2 == a.d2 && idx < a.idx))) { a.d2 = d2; a.idx = idx; }
}

template <int STEP>
__device__ __forceinline__ VoxBest vox_best_members(const float *__restrict__ xyz, const int *__restrict__ order, int first, int end, const double mean[3])
{
    VoxBest best{ 0.0, -1 };
    for (int m = first; m < end; m += 4 * STEP) {
        int idx[4];
        float v[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) idx[u] = m + u * STEP < end ? order[m + u * STEP] : -1;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int a = 0; a < 3; ++a) v[u][a] = idx[u] >= 0 ? xyz[3 * (long long)idx[u] + a] : 0.0f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double dx = (double)v[u][0] - mean[0], dy = (double)v[u][1] - mean[1], dz = (double)v[u][2] - mean[2];
            vox_best_merge(best, (dx * dx + dy * dy) + dz * dz, idx[u]);
        }
    }
    return best;
}

template <int WIDTH>
__device__ __forceinline__ void vox_best_butterfly(VoxBest &best)
{
#pragma unroll
    for (int o = WIDTH / 2; o > 0; o >>= 1) {
        const double d2 = __shfl_xor(best.d2, o, 64);
        const int idx = __shfl_xor(best.idx, o, 64);
        vox_best_merge(best, d2, idx);
    }
}

__global__ __launch_bounds__(VOX_THREADS) void k_voxel_rep(const float *__restrict__ xyz, const int *__restrict__ order, const int *__restrict__ row_start,
                                                           int n_rows, const float *__restrict__ out_xyz, int *__restrict__ out_rep)
{
    const long long row = ((long long)blockIdx.x * VOX_THREADS + threadIdx.x) / VOX_GROUP;
    const int j = threadIdx.x & (VOX_GROUP - 1);
    const bool live = row < n_rows;
    int b = 0, e = 0;
    double mean[3] = { 0.0, 0.0, 0.0 };
    if (live) {
        b = row_start[row]; e = row_start[row + 1];
        for (int a = 0; a < 3; ++a) mean[a] = (double)out_xyz[3 * row + a];
    }
    const bool small = e - b <= VOX_CHUNK;
    VoxBest best{ 0.0, -1 };
    if (small) best = vox_best_members<VOX_GROUP>(xyz, order, b + j, e, mean);
    vox_best_butterfly<VOX_GROUP>(best);
    if (live && small && j == 0) out_rep[row] = best.idx;
}

__global__ __launch_bounds__(VOX_THREADS) void k_voxel_rep_long(const float *__restrict__ xyz, const int *__restrict__ order, const int *__restrict__ row_start,
                                                                const long long *__restrict__ chunk_off, int n_rows, const float *__restrict__ out_xyz,
                                                                double *__restrict__ part_d2, int *__restrict__ part_idx)
{
    const int lane = threadIdx.x & 63;
    const long long total = chunk_off[n_rows], n_waves = (long long)gridDim.x * (VOX_THREADS / 64);
    for (long long w = (long long)blockIdx.x * (VOX_THREADS / 64) + (threadIdx.x >> 6); w < total; w += n_waves) {
        const int r = vox_row_of_chunk(chunk_off, n_rows, w);
        const long long b = (long long)row_start[r] + (w - chunk_off[r]) * VOX_CHUNK;
        const int e = (int)min(b + VOX_CHUNK, (long long)row_start[r + 1]);
        double mean[3];
        for (int a = 0; a < 3; ++a) mean[a] = (double)out_xyz[3 * (long long)r + a];
        VoxBest best = vox_best_members<64>(xyz, order, (int)b + lane, e, mean);
        vox_best_butterfly<64>(best);
        if (lane == 0) { part_d2[w] = best.d2; part_idx[w] = best.idx; }
    }
}

__global__ __launch_bounds__(VOX_THREADS) void k_voxel_rep_finish_long(const long long *__restrict__ chunk_off, int n_rows, const double *__restrict__ part_d2,
                                                                       const int *__restrict__ part_idx, int *__restrict__ out_rep)
{
    const long long r = (long long)blockIdx.x * VOX_THREADS + threadIdx.x;
    if (r >= n_rows) return;
    const long long c0 = chunk_off[r], c1 = chunk_off[r + 1];
    if (c1 == c0) return;
    VoxBest best{ 0.0, -1 };
    for (long long c = c0; c < c1; ++c) vox_best_merge(best, part_d2[c], part_idx[c]);
    out_rep[r] = best.idx;
}

#endif  // __HIPCC__
}  // namespace oa
