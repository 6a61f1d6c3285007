// oa_icp.hip -- C-ABI (include/oa_icp.h) over the gfx950 kernels in oa_kernels.hpp.
//
// Host side of the drop-in boundary: context lifetime, uploads/packing, launch geometry, the device-resident
// iterate loop and its split-phase form for one-process-per-GPU sharding.  No CPU fallback lives here: every
// compute entry point needs a usable HIP device and fails loudly otherwise.
#include <cstring>
#include <dlfcn.h>
// librccl is loaded with dlopen on first use (liboa_icp.so has no link dependency on it); a ROCm install without the
// RCCL development headers still builds this file from the handful of declarations the exchange needs
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
typedef struct ncclComm *ncclComm_t;
typedef enum { ncclSuccess = 0, ncclInProgress = 7 } ncclResult_t;
typedef enum { ncclFloat64 = 8, ncclDouble = 8 } ncclDataType_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
#endif

#include "oa_all.hpp"                // every kernel header + oa_families.hpp: the heavy templates are `extern` here, compiled in oa_fam_*.hip
#include "oa_sort.hpp"
#include "oa_voxel.hpp"
#include "oa_sample.hpp"
#include "oa_orient.hpp"
#include "oa_deviation.hpp"
#include "oa_boundary.hpp"
#include "oa_tunables.hpp"            // every OA_* knob: read once, oa_ctx::tune (plain C++)
#include "oa_devbuf.hpp"              // DevBuf<T>: the owner of every block of device memory (plain C++)
#include "../../include/oa_icp.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <thread>
#include <type_traits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#define OA_EXPORT extern "C" __attribute__((visibility("default")))
// a multi-device parent (oa_create_multi) routes the call to every child / to its first child
#define OA_ROUTE_ALL(c, call)                                                                  \
    if ((c) && !(c)->subs.empty()) {                                                           \
        for (oa_ctx *sub : (c)->subs) { const int rc_ = (call); if (rc_) return rc_; }         \
        return OA_OK;                                                                          \
    }
// uploads and index builds: the children work at the same time, one host thread each, when they sit on different GPUs
#define OA_ROUTE_ALL_PAR(c, call)                                                              \
    if ((c) && !(c)->subs.empty()) return route_all_parallel((c), [&](oa_ctx *sub) -> int { return (call); });
#define OA_ROUTE_FIRST(c, call)                                                                \
    if ((c) && !(c)->subs.empty()) { oa_ctx *sub = (c)->subs[0]; return (call); }
#define OA_NOT_MULTI(c, what)                                                                  \
    if ((c) && !(c)->subs.empty())                                                             \
        return fail(OA_E_STATE, what ": not available on a multi-device context (use a single-device one)");

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        const hipError_t e_ = (hipError_t)(expr);       /* (a DevBuf's alloc returns the code as an int) */ \
        if (e_ != hipSuccess)                                                                          \
            return fail(OA_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Device allocations go through a small process-wide cache keyed by (device, size): hipFree costs ~135 us a call on
// this stack (it synchronises the device), and an upload frees and reallocates ~25 buffers of unchanged size -- more
// than half of oa_set_target + oa_set_source at 1M points.  A released block is kept for the next request of the same
// size; blocks that sit unused for CACHE_MAX_AGE releases, or push the cache past its cap, are really freed.
// The library is a guest in somebody else's process (Blender): the cap is 256 MiB or the library's own peak of live bytes,
// whichever is larger (OA_DEV_CACHE_MB sets a fixed cap, OA_DEV_CACHE=0 switches the cache off), and when the last context is
// destroyed everything is freed.
// Releases are STREAM ORDERED, not device-synchronising: a block goes back tagged with the stream of the context that
// used it (tl_stream, set by use_device).  The next owner on the same stream needs no wait at all (stream order); an
// owner on another stream first waits for the releasing stream (rare: two contexts trading blocks).  Only a real hipFree
// synchronises (the runtime's own rule).  No events: recording one per release cost more than the device synchronisation
// it replaced on an idle device (a whole alignment call of 2562 points: 0.46 -> 0.64 ms).
thread_local hipStream_t tl_stream = nullptr;
thread_local bool tl_stream_known = false;

struct DevCache {
    struct Block { void *p; size_t bytes; int device; unsigned long long stamp; hipStream_t stream; bool settled; };
    std::mutex mu;
    std::vector<Block> free_blocks;
    std::unordered_map<void *, std::pair<size_t, int>> live;    // pointer -> (bytes, device)
    size_t cached_bytes = 0;
    unsigned long long clock = 0;
    int contexts = 0;                                           // live oa_ctx objects (single-device ones)
    static constexpr unsigned long long CACHE_MAX_AGE = 512;

    const oa_tune::CacheTunables tune = oa_tune::read_cache_tunables();   // (at the process's first allocation: dev_cache())
    const bool enabled = tune.enabled;                          // OA_DEV_CACHE=0: plain hipMalloc / hipFree
    const bool cap_given = tune.cap_given;
    const size_t max_bytes = (size_t)tune.cap_mb << 20;
    // The cap follows what the process has had allocated AT ONCE (round 6): a 1.96M-triangle mesh is ~0.5 GB of images, lists and
    // trees, and with a fixed 256 MiB every re-upload of it really freed and really allocated most of that -- 2.9 of the 4.8 ms of
    // oa_set_target_mesh.  Idle, the cache never holds more than the library already needed live; an explicit OA_DEV_CACHE_MB wins.
    size_t live_bytes = 0, peak_live = 0;
    size_t cap() const { return cap_given ? max_bytes : std::max(max_bytes, peak_live); }

    hipError_t alloc(void **out, size_t bytes)
    {
        if (bytes == 0) bytes = 1;
        if (!enabled) return hipMalloc(out, bytes);
        int dev = 0;
        (void)hipGetDevice(&dev);
        {
            std::unique_lock<std::mutex> lk(mu);
            for (size_t i = 0; i < free_blocks.size(); ++i)
                if (free_blocks[i].bytes == bytes && free_blocks[i].device == dev) {
                    const Block b = free_blocks[i];
                    *out = b.p;
                    cached_bytes -= bytes;
                    free_blocks[i] = free_blocks.back();
                    free_blocks.pop_back();
                    live[*out] = { bytes, dev };
                    live_bytes += bytes; peak_live = std::max(peak_live, live_bytes);
                    lk.unlock();
                    // same stream: stream order is enough.  Another stream (or none known): whatever the releasing
                    // stream still has in flight must finish first
                    if (!b.settled && !(tl_stream_known && b.stream == tl_stream))
                        if (hipStreamSynchronize(b.stream) != hipSuccess) { (void)hipGetLastError(); (void)hipDeviceSynchronize(); }
                    return hipSuccess;
                }
        }
        hipError_t e = hipMalloc(out, bytes);
        if (e != hipSuccess) {                                     // out of memory: drop the cache and retry once
            (void)hipGetLastError();
            trim(0, 0);
            e = hipMalloc(out, bytes);
        }
        if (e == hipSuccess) { std::lock_guard<std::mutex> lk(mu); live[*out] = { bytes, dev }; live_bytes += bytes; peak_live = std::max(peak_live, live_bytes); }
        return e;
    }

    // settled: the caller has already synchronised the device (oa_destroy) -- nothing can still be using the block
    void release(void *p, bool settled = false)
    {
        if (!p) return;
        if (!enabled) { (void)hipFree(p); return; }
        std::lock_guard<std::mutex> lk(mu);
        auto it = live.find(p);
        if (it == live.end()) { (void)hipFree(p); return; }
        Block b{ p, it->second.first, it->second.second, ++clock, tl_stream, settled };
        live.erase(it);
        live_bytes -= std::min(live_bytes, b.bytes);
        if (b.bytes > cap()) { (void)hipFree(p); return; }         // would not fit under the cap anyway (hipFree synchronises)
        if (!settled && !tl_stream_known) { (void)hipDeviceSynchronize(); b.settled = true; }   // no stream to order against
        free_blocks.push_back(b);
        cached_bytes += b.bytes;
        trim_locked(cap(), CACHE_MAX_AGE);
    }

    // a stream is about to be destroyed (its device has been synchronised): its blocks have nothing in flight any more
    void stream_gone(hipStream_t s)
    {
        std::lock_guard<std::mutex> lk(mu);
        for (Block &b : free_blocks) if (b.stream == s) { b.settled = true; b.stream = nullptr; }
    }

    void trim(size_t cap, unsigned long long max_age) { std::lock_guard<std::mutex> lk(mu); trim_locked(cap, max_age); }

    void trim_locked(size_t cap, unsigned long long max_age)
    {
        // oldest first, so that what stays is what was released last
        std::sort(free_blocks.begin(), free_blocks.end(), [](const Block &a, const Block &b) { return a.stamp < b.stamp; });
        size_t i = 0;
        while (i < free_blocks.size()) {
            const bool old = clock - free_blocks[i].stamp > max_age;
            if (old || cached_bytes > cap) {
                (void)hipFree(free_blocks[i].p);                   // synchronises the device
                cached_bytes -= free_blocks[i].bytes;
                free_blocks.erase(free_blocks.begin() + (long)i);
            } else ++i;
        }
    }

    void context_created() { std::lock_guard<std::mutex> lk(mu); ++contexts; }
    void context_destroyed()
    {
        std::lock_guard<std::mutex> lk(mu);
        if (--contexts > 0) return;
        contexts = 0;
        trim_locked(0, 0);                                         // last context gone: give everything back
        peak_live = live_bytes;
    }
};

DevCache &dev_cache()
{
    static DevCache *cache = new DevCache();                      // never destroyed: the HIP runtime may already be gone at exit
    return *cache;
}

}  // namespace

int oa::dev_block_alloc(void **out, size_t bytes) { return (int)dev_cache().alloc(out, bytes); }
void oa::dev_block_release(void *p, bool settled) { dev_cache().release(p, settled); }

namespace {

// every block has one owner (oa_devbuf.hpp): a member of oa_ctx's lifetime groups, or a local released on every exit path (DevTmp)
using oa::DevBuf;
template <typename T> using DevTmp = DevBuf<T>;
template <typename T> hipError_t dev_malloc(DevBuf<T> *b, size_t bytes) { return (hipError_t)b->alloc_bytes(bytes); }

// Host threads of a multi-device context.  One PERSISTENT worker per listed GPU (children that share a GPU share a
// worker and stay sequential): uploads and index builds (20+ ms of copies, sorts and builds per device at 1M) run on all
// GPUs at the same time, and oa_run hands every worker the whole loop of its device -- each GPU is fed by its own
// thread, so the enqueue cost per iteration does not grow with the number of GPUs.  Round 2 spawned fresh std::threads
// per upload call and enqueued every device's iteration from the calling thread (~50 runtime calls per iteration at 8
// GPUs).  OA_MULTI_THREADS: -1 (default) as above, 0 = everything on the calling thread, 1 = one worker per CHILD even
// when children share a GPU (test hook: the threaded paths on a one-GPU box).
struct WorkerPool {
    struct Worker {
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        std::function<int()> job;
        bool has_job = false, done = true, quit = false;
        int rc = 0;
        std::string err;
    };
    std::vector<std::unique_ptr<Worker>> workers;

    static void loop(Worker *w)
    {
        for (;;) {
            std::function<int()> job;
            {
                std::unique_lock<std::mutex> lk(w->mu);
                w->cv.wait(lk, [w] { return w->has_job || w->quit; });
                if (w->quit) return;
                job = std::move(w->job);
                w->has_job = false;
            }
            g_err.clear();
            const int rc = job();
            {
                std::lock_guard<std::mutex> lk(w->mu);
                w->rc = rc;
                w->err = rc ? g_err : std::string();
                w->done = true;
            }
            w->cv.notify_all();
        }
    }

    void start(size_t n)
    {
        while (workers.size() < n) {
            workers.emplace_back(new Worker());
            Worker *w = workers.back().get();
            w->th = std::thread(loop, w);
        }
    }

    // f(k) for k = 0 .. n-1: k = 0 on the calling thread, the others on workers 0 .. n-2.  The first failure (lowest k)
    // wins: its code is returned and its message becomes this thread's oa_last_error().
    template <typename F> int run(size_t n, F f)
    {
        if (n == 0) return OA_OK;
        start(n - 1);
        for (size_t k = 1; k < n; ++k) {
            Worker *w = workers[k - 1].get();
            {
                std::lock_guard<std::mutex> lk(w->mu);
                w->job = [f, k]() -> int { return f(k); };
                w->has_job = true;
                w->done = false;
            }
            w->cv.notify_all();
        }
        int rc0 = f(0);
        std::string err0 = rc0 ? g_err : std::string();
        for (size_t k = 1; k < n; ++k) {
            Worker *w = workers[k - 1].get();
            std::unique_lock<std::mutex> lk(w->mu);
            w->cv.wait(lk, [w] { return w->done; });
            if (!rc0 && w->rc) { rc0 = w->rc; err0 = w->err; }
        }
        if (rc0) g_err = err0;
        return rc0;
    }

    ~WorkerPool()
    {
        for (auto &w : workers) {
            { std::lock_guard<std::mutex> lk(w->mu); w->quit = true; }
            w->cv.notify_all();
            if (w->th.joinable()) w->th.join();
        }
    }
};

template <typename F> int route_all_parallel(oa_ctx *c, F f);

}  // namespace

// Device memory is owned by lifetime.  A group's members are handles and plain values with default initialisers:
// the upload that ends the lifetime assigns `{}` to the group, the context's destructor releases what is left.
// The resident target: set_target_common forgets all of it.
struct oa_target {
    int nt = 0, n_groups_pad = 0;
    DevBuf<float> d_tgt_xyz;
    DevBuf<float4> d_tg;
    DevBuf<float4> d_tf;             // filter image, level 1: 3 float4 per group (k_nn_search_filtered)
    DevBuf<float4> d_tf3;            // filter image, level 2: 2 float4 per group
    // the same images in the order of the coordinate along the cloud's longest axis (k_nn_search_sorted, round 5)
    DevBuf<float4> d_tfs, d_tf3s, d_tgs;   // 3 / 2 / 3 float4 per group of 4 sorted positions
    DevBuf<float4> d_tmw;            // level 0's pair images, 1 float4 per group: {m, w} of positions (0, 1) and (2, 3) (oa_pairgap.hpp)
    DevBuf<float4> d_toct;           // level 0's images of SORTED_IMAGE_V positions each, 3 float4 per 4 images: their {mm}, {ww}, {ws} (oa_octgap.hpp)
    float oct_c = 0.0f;              // the cap d_toct was built with (0 while there are no images); k_sorted_point_setup gets it at launch
    DevBuf<int4> d_tidx;             // original index of every sorted position
    DevBuf<oa::half8> d_tfm;         // the MFMA experiment's image of the target
    bool filter_ok = false;
    // uniform grid (k_nn_search_grid)
    bool grid_ok = false;
    oa::GridParams gp;
    int n_cells = 0;
    DevBuf<int> d_cell_start;
    DevBuf<float4> d_sorted;
    DevBuf<float> d_safe_by_idx;     // vertex grid: safe2 per target vertex (original index); allocated with the grid, filled by build_safe_radii
    bool safe_ok = false;            // ... and filled
    long long target_iters = 0;      // accumulating grid searches enqueued since the target was set
    // surface mode (closest point on triangle, oa_tri.hpp)
    bool surface = false, tri_grid_ok = false;
    int n_tris = 0;
    DevBuf<float4> d_tri9;
    DevBuf<int> d_tris;              // the mesh's vertex indices, n_tris x 3 (the pseudo-normals are built from them, oa_deviation.hpp)
    // angle-weighted pseudo-normals of the mesh (oa_deviation / oa_get_mesh_pseudonormals): built at the first signed call
    bool pn_ok = false;
    DevBuf<double> d_pn_face;        // n_tris x 3: unit face normals
    DevBuf<float> d_pn_vertex, d_pn_edge;   // nt x 3; n_tris x 3 edges x 3
    oa::GridParams tgp;
    DevBuf<int> d_tcell_start;
    DevBuf<float4> d_tcell_rec;      // two float4 per cell-list entry: {disc centre, radius} {unit normal, triangle index}
    long long n_tri_entries = 0;     // entries of the triangle grid's cell lists
    double tri_mean_diag = 0.0;      // mean bounding-box diagonal of the triangles (the cell sizes are multiples of it)
    // the settled-pose search (oa_tri_fine.hpp): a sparse fine grid with inflated lists of whole triangles
    bool tri_fine_ok = false;
    oa::FineParams tfp;
    DevBuf<uint4> d_tfine_table;
    DevBuf<float4> d_tfine_rec;
    long long n_fine_entries = 0;
    // seed + neighbours settle a query (oa_tri_ring.hpp): per triangle its neighbours' indices; the accept radius lives in d_tri9
    DevBuf<int> d_tri_ring;
    bool tri_ring_ok = false;
    long long tri_iters = 0;         // loop searches enqueued since the mesh was set
    // bounding-box trees (oa_bvh.hpp): over the vertices, and over the triangles in surface mode
    bool bvh_ok = false, tbvh_ok = false;
    oa::BvhParams bvh, tbvh;
    DevBuf<float4> d_bvh_box, d_bvh_prims, d_tbvh_box, d_tbvh_prims;
    DevBuf<float> d_tgt_n;           // normal-angle rejection (extension)
    DevBuf<float> d_tgt_feat;        // oa_target_fpfh(keep): nt x 33 descriptors of the resident target, or empty
    // oa_target_boundary: the target's rim (oa_boundary.hpp).  The masks are built on demand (the cloud's again when its normals or (k, angle) change)
    DevBuf<unsigned char> d_bnd_vmask, d_bnd_emask;                 // nt bytes; n_tris bytes (mesh targets)
    bool bnd_ok = false;
    int bnd_built_k = 0; double bnd_built_angle = 0.0;              // what a cloud's mask was built with
    float bnd_built_r2 = INFINITY;                                  // ... and the neighbour radius' square then in force (+inf: none)
    long long bnd_n_vertices = 0, bnd_n_edges = 0;                  // OA_STAT_BOUNDARY_VERTICES / _EDGES
    DevBuf<int> d_corner_order; DevBuf<long long> d_corner_row;     // the mesh's corners by vertex (CSR rows): the pseudo-normals and the
    bool corner_ok = false;                                         // boundary share them
    long long cleaned = 0;                                          // OA_STAT_TARGET_CLEANED: what oa_target_outliers(apply) removed to get here
};

// The source shard: source_reset forgets all of it.
struct oa_source {
    int ns = 0, ns_pad = 0, R = 4;   // R: tune.nn_r, or chosen from the shard size
    DevBuf<float4> d_src4;
    DevBuf<unsigned long long> d_keys;
    DevBuf<int> d_prev;              // nearest index of the previous search (seed), -1 = none
    DevBuf<float4> d_win;            // vertex mode: per slot, the last winner's coordinates + index in .w (-1 = none)
    DevBuf<uint2> d_wsafe;           // vertex grid: per slot {index, safe2 bits} of a winner the grid scan found (k_grid_safe_radius); 0xFF.. = none.  Sized by the source, held only against a vertex target: set_target_common frees or allocates it too
    DevBuf<int> d_sel;               // vertex index held by each source slot
    DevBuf<float4> d_src4o;          // the same points in the caller's (vlist) order -- only oa_make_pairs needs it
    DevBuf<int> d_perm;              // sorted slot -> caller-order slot (empty: not sorted)
    DevBuf<int> d_members;           // shard of a spatially sharded selection: position in the whole selection of every caller-order slot (ascending); empty = shard_begin + slot
    long long shard_begin = 0;
    DevBuf<int> d_pos;               // oa_make_pairs on a shard: whole-selection position of every pair
    std::vector<int> h_members;      // host copy of d_members (children of a multi-device context)
    DevBuf<float4> d_prec;           // k_sorted_point_setup: k_nn_search_sorted's point records, 3 float4 per slot in the order its lanes read them + a fourth array, one float4 per lane and pair of its points (oa_quadgap.hpp) (OA_NN_WAVE_ORDER=0: the slots' own order)
    int prec_cap = 0;                // slots d_prec holds
    int homes_cap = 0;               // blocks of source points d_homes holds (two ints each: home split, home tile)
    DevBuf<int> d_homes, d_qcnt;     // k_nn_search_sorted's work queue (oa_kernels.hpp): per block of source points its own split; the queues' counters
    long long src_n_verts = 0;
    DevBuf<int> d_todo_list, d_todo_count;   // d_todo_count: {entries, most per wave} of the hand-over list; from TODO_WORDS on: the two counter sets of d_ulist
    DevBuf<int> d_ulist;             // surface mode: the queries the front search (k_tri_settle) did not settle -> k_tri_search_grid (oa_tri.hpp: ulist_*)
    int u_slot = 0;                  // which of the two counter sets the next front launch fills (it zeroes the other one)
    DevBuf<float> d_src_n;           // normal-angle rejection (extension)
    DevBuf<float> d_w;               // oa_set_source_weights: one weight per slot (gathered through d_sel), or empty
    DevBuf<uint32_t> d_rkeys;        // one residual key per slot (k_residual_keys), allocated when a loop with oa_set_robust_auto or oa_set_trim on begins
    oa::BvhParams sbvh{};            // oa_set_reciprocal: the box tree over the selected source points (align-local, primitive index = slot) ...
    DevBuf<float4> d_sbvh_box, d_sbvh_prims;
    bool sbvh_ok = false;            // ... built by the first step with the check on
    DevBuf<unsigned char> d_recip_ok;   // k_recip_check's verdict, one byte per slot (the trim's and the boundary's go into it too)
    DevBuf<uint32_t> d_trim_sorted; DevBuf<int> d_trim_order; DevBuf<char> d_trim_tmp;   // oa_set_trim, estimated share: the sorted keys, their order, the sort's scratch
    DevBuf<double> d_trim_tiles; DevBuf<oa::TrimTileMin> d_trim_min;                       // ... the scan's tile sums / bases and the tiles' minima
    double pivot[3] = { 0, 0, 0 };
    // make_pairs scratch (sized to ns)
    int emit_cap = 0;
    DevBuf<unsigned char> d_valid;
    DevBuf<float> d_b;
    DevBuf<double> d_dist;
    DevBuf<int> d_counts;
    DevBuf<long long> d_offsets;
    DevBuf<double> d_A, d_B;
};

struct oa_ctx {
    const oa_tune::Tunables tune = oa_tune::read_tunables();   // configuration: fixed for the context's life.  Everything below is state
    int device = 0;
    int n_cu = 256;
    hipStream_t own_stream = nullptr, stream = nullptr;
    oa_target tgt;
    oa_source src;
    // Context-wide from here on: settings (they survive uploads and oa_set_matrices), the loop's state, buffers no upload resizes,
    // statistics -- and what build_filter found: a non-finite target leaves the old values in place, unread while !filter_ok
    int sax[3] = { 0, 1, 2 };        // the sorted images' axes: longest (sorted along), second, thinnest
    int fax[3] = { 0, 1, 2 };
    double bb_lo[3] = { 0, 0, 0 }, bb_hi[3] = { 0, 0, 0 };
    float tc[3] = { 0, 0, 0 };
    double qmax = 0.0;
    double mfma_sigma = 1.0;
    int grid_mode = -1;              // -1 auto, 0 never, 1 whenever possible: tune.nn_grid at oa_create, then oa_set_search_mode
    double last_pn_ms = 0.0;         // host time of the last pseudo-normal build
    // both uploads reset these three and loop_active, each explicitly: they speak of the pair of target and source
    bool seeded = false;             // a search has run since the last set_source / set_target (seeds exist)
    bool win_seeds = false;          // an accumulation has written winner records since the last upload / oa_reset_seeds
    bool normals_on = false;
    int last_queue_wgs = 0;          // OA_STAT_BRUTE_QUEUE_WGS
    double cos_min = -2.0;           // normal-angle rejection (extension)
    int last_plane_rank = 0;         // OA_STAT_PLANE_RANK: eigenvalues the last plane solve kept (loop or oa_point_to_plane)
    int metric = OA_METRIC_POINT;    // oa_set_metric: what the loop minimises
    double gicp_eps = 1e-3;          // oa_set_gicp: the small eigenvalue of the GICP metric's covariances
    float nbr_radius = 0.f;          // oa_set_neighbor_radius: what limits the neighbourhoods of oa_target_knn and its three consumers; 0 = off
    // weighted steps: a pair's weight is w_vertex * psi(residual).  Off (every weight 1, the unweighted kernels) unless set
    int loss = OA_LOSS_NONE;         // oa_set_robust
    double robust_c = 0.0;           // ... its scale, world units
    double last_weight_sum = 0.0;    // OA_STAT_WEIGHT_SUM
    // oa_set_robust_auto: the loss's scale from each step's own residuals, c = max(robust_c * q, robust_cmin) -- robust_c is then
    // the multiplier m.  Off while robust_p == 0; inert while the loss is NONE
    double robust_p = 0.0, robust_cmin = 0.0;
    DevBuf<uint32_t> d_sel_hist;     // the radix select's SEL_LEVELS histograms
    double last_robust_c = 0.0;      // OA_STAT_ROBUST_SCALE: the c the last step used
    // oa_set_reciprocal: keep a pair only if it is mutual (oa_recip.hpp)
    bool recip_on = false;
    double recip_ratio = 1.0;
    int src_shards = 1;              // shard_count of the last oa_set_source: a shard cannot see the other shards' source points
    DevBuf<unsigned> d_recip_count;  // k_recip_check's counters (RECIP_COUNT_WORDS): word 2 = slots the last step rejected
    // oa_set_trim: every step keeps its best pairs only (oa_trim.hpp).  The verdict goes into src.d_recip_ok, the keys into
    // src.d_rkeys; the rest is the trim's own, allocated when a loop (or oa_make_pairs) with the setting on begins
    double trim_fraction = 0.0;      // 0 = off, (0, 1] = the share kept, OA_TRIM_AUTO = estimated every step
    double trim_min = 0.3, trim_lambda = 2.0;
    DevBuf<oa::DevTrim> d_trim;      // its state between the launches, and the last step's figures (OA_STAT_TRIM_*)
    DevBuf<uint32_t> d_trim_hist;    // fixed share: the select's SEL_LEVELS histograms
    // oa_set_reject_boundary: drop pairs on the target's rim (the masks: oa_target)
    bool bnd_on = false;
    int bnd_k = 16;
    double bnd_angle = 90.0;
    double last_bnd_ms = 0.0;                                       // host time of the last mask build
    DevBuf<unsigned> d_bnd_count;                                   // k_boundary_verdict's counters (BND_COUNT_WORDS): word 2 = slots the last step rejected
    // launch geometry for k_nn_search
    int n_splits = 1, acc_blocks = 1;
    int n_splits_seeded = 1;         // k_nn_search_sorted once the winner records hold seeds: more, shorter splits (plan_geometry)
    int tile_groups = oa::FTILE_GROUPS;   // LDS tile of k_nn_search_filtered: 256 groups, 64 for small targets
    double d_pivot0 = 0.0;           // initial distance pivot for the next loop / one-shot (see DevState::d_pivot)
    // device state
    oa::DevState h_state;
    DevBuf<oa::DevState> d_state;
    bool have_mats = false, loop_active = false;
    oa::StepRecord *d_hist = nullptr;       // device view of h_hist_map: the solve kernel writes the records straight into host memory
    oa::StepRecord *h_hist_map = nullptr;   // pinned, device-mapped history (read after a stream sync, no copy)
    oa::DevState *h_state_pin = nullptr;    // pinned staging of DevState (pageable copies cost ~30 us each way)
    char *h_scratch = nullptr;              // pinned scratch for small read-backs (read_small)
    char *h_result = nullptr;               // pinned, device-mapped: kernels store small results here (result_buffer)
    void *d_result_view = nullptr;
    double last_exchange_us = 0.0;        // mean exchange wait per iteration of the last loop (fill_report; OA_STAT_EXCHANGE_US)
    std::vector<double> h_search_ms;      // search time of every iteration of the last loop (fill_report; oa_get_search_ms)
    std::vector<oa::StepRecord> h_hist;   // host copy of the executed iterations' records, filled by fill_report
    bool h_hist_valid = false;
    int max_records = 0;
    DevBuf<double> d_partials, d_sums, d_solve;
    int iter_enq = 0;                       // iterations enqueued since the loop began
    int fast_iters = 0;                     // ... of which the grid search finished its own leftovers and accumulated (OA_STAT_FAST_ITERATIONS)
    bool fast_prev = false;                 // what the last iteration's grid search did
    int last_acc_path = 0, last_acc_rows = 0;   // OA_STAT_ACC_PATH / _ROWS: the last step's accumulation (OA_ACC_*) and the reduce launch's first row count
    int last_todo_wave_max = -1;            // most queries one wave handed over in the last iteration the host heard of (-1: unknown)
    // timing
    std::vector<hipEvent_t> ev;
    int ev_used = 0;
    hipEvent_t ev_loop0 = nullptr, ev_loop1 = nullptr;
    bool poll_mapped = false;           // the device can write h_poll (DevState::host_halt is set): else the kernels never report their progress there
    int32_t *h_poll = nullptr;          // pinned, device-mapped {halt, n, hand-over entries, most per wave, -, iteration whose exchange the stream has reached (k_reduce_partials), -, -}: the kernels mirror them here for the enqueuing host
    bool time_events = true;            // hipEvent pair around every search (brute force); else GPU-side stamps (see iter_fused)
    double wall_clock_khz = 100000.0;   // rate of wall_clock64()
    oa_settings settings;
    bool iterate_mode = false;          // the active loop was opened by oa_iterate (small history ring)
    // multi-device (oa_create_multi).  The parent only routes: uploads go to every child (target replicated, source
    // sharded child i of n), the loop drives all children and the exchange below joins their sums every iteration.
    std::vector<oa_ctx *> subs;         // parent: one child per entry of the device list
    struct oa_exchange *xch = nullptr;  // parent: owns it; child: the parent's
    oa_ctx *parent = nullptr;
    int rank = 0, world = 1;            // child: its place in the device list
    std::vector<std::vector<int>> groups;   // parent: children per host thread in the LOOP (one group per GPU, see WorkerPool)
    std::vector<std::vector<int>> upload_groups;   // ... and in uploads / index builds (OA_MULTI_THREADS=1: one per child)
    WorkerPool *pool = nullptr;         // parent: the persistent host threads of groups 1 .. n-1 (group 0 = the caller)
    double last_nn_ms = 0.0;            // child: search time of the last oa_run on this device (OA_STAT_NN_MS_MIN / _MAX)
    double enq_ns = 0.0;                // child: host time spent enqueuing its iterations in the last loop
    long long enq_iters = 0;
};

namespace {

// d_todo_count: TODO_WORDS ints for the tree's hand-over list, then two sets of the front search's list counters (ulist_*)
constexpr int TODO_WORDS = 32, UCOUNT_WORDS = oa::ULIST_PARTS * oa::ULIST_STRIDE, TODO_COUNT_INTS = TODO_WORDS + 2 * UCOUNT_WORDS;
[[maybe_unused]] inline int *ucount_set(const oa_ctx *c, int slot) { return c->src.d_todo_count + TODO_WORDS + slot * UCOUNT_WORDS; }

int use_device(oa_ctx *c)
{
    HIPCHK(hipSetDevice(c->device));
    tl_stream = c->stream; tl_stream_known = true;              // releases of device blocks are ordered on this stream
    return OA_OK;
}

// which GPU a device pointer lives on (-1: not a device pointer the runtime knows)
int pointer_device(const void *ptr)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return at.type == hipMemoryTypeDevice ? at.device : -1;
}

template <typename F> int route_all_parallel(oa_ctx *c, F f)
{
    const size_t ng = c->upload_groups.size();
    if (ng <= 1 || !c->pool) {
        for (oa_ctx *sub : c->subs) { const int rc = f(sub); if (rc) return rc; }
        return OA_OK;
    }
    return c->pool->run(ng, [c, f](size_t g) -> int {
        for (int i : c->upload_groups[g]) { const int rc = f(c->subs[(size_t)i]); if (rc) return rc; }
        return OA_OK;
    });
}

void plan_geometry(oa_ctx *c)
{
    if (c->src.ns <= 0 || c->tgt.nt <= 0) return;
    const int src_blocks = c->src.ns_pad / (oa::NN_THREADS * c->src.R);
    // small targets: quarter-size tiles give 4x more (and 4x shorter) workgroups; the unfiltered kernel keeps 256
    c->tile_groups = (c->tgt.filter_ok && c->tune.nn_filter && c->tgt.nt <= 65536 && !c->tune.nn_bigtile) ? 64 : oa::FTILE_GROUPS;
    const int tiles_total = c->tgt.n_groups_pad / c->tile_groups;
    // workgroups wanted: ~2e5 pairs each (below that the prologue and the atomicMin merge dominate), at most 64 per CU
    const double pairs = (double)c->src.ns * (double)c->tgt.nt;
    const int want_auto = (int)std::min((double)c->n_cu * 64.0, std::max((double)c->n_cu * 2.0, pairs / 2e5));
    const int want = c->tune.nn_target_blocks == oa_tune::UNSET ? want_auto : c->tune.nn_target_blocks;
    int splits = (want + src_blocks - 1) / src_blocks;
    splits = std::max(1, std::min(splits, tiles_total));
    if (splits > 8) splits = std::min(tiles_total, ((splits + 7) / 8) * 8);   // multiple of 8: one XCD per split residue
    const int forced = c->tune.nn_splits;
    if (forced > 0) splits = std::min(forced, tiles_total);
    c->n_splits = splits;                                          // the kernels cut the tiles into exactly this many ranges (split_range)
    // k_nn_search_sorted with seeds: a workgroup's points reach levels 1-3 only in the split that holds their own slab, so short
    // splits (>= 3 tiles each, up to 512 workgroups per CU in the grid) even the workgroups out and keep a split's few tiles in
    // its XCD's L2: 1M <-> 1M 37.0 -> 34.5 ms, the 125k shard 5.14 -> 4.74 ms (tools/sweep_sorted_splits.py,
    // profiles/r05y_sorted_splits.txt).  WITHOUT seeds every split has to find a best of its own first, and more splits cost
    // (52 -> 80 ms at 136): the first search of a loop keeps the count above.
    int seeded = std::min(tiles_total / 3, (c->n_cu * 512 + src_blocks - 1) / src_blocks);
    if (seeded > 8) seeded = std::min(tiles_total, ((seeded + 7) / 8) * 8);
    seeded = std::max(splits, seeded);
    const int forced_seeded = c->tune.nn_splits_seeded;
    if (forced > 0) seeded = splits;
    if (forced_seeded > 0) seeded = std::min(forced_seeded, tiles_total);
    c->n_splits_seeded = seeded;
    const int acc_cap = std::max(1, std::min(oa::ACC_MAX_BLOCKS, c->tune.acc_blocks));
    c->acc_blocks = std::max(1, std::min(acc_cap, (c->src.ns + oa::ACC_THREADS - 1) / oa::ACC_THREADS));
}

int ensure_common(oa_ctx *c)
{
    if (!c->d_state) HIPCHK(dev_malloc(&c->d_state, sizeof(oa::DevState)));
    // (sized for the widest user: the plane metric's rows of NSUMS_PLANE, one per workgroup of k_pair_accumulate_plane)
    static_assert(oa::NSUMS_PLANE * oa::PLANE_MAX_BLOCKS >= oa::NSUMS * oa::ACC_MAX_BLOCKS, "d_partials");
    if (!c->d_partials) HIPCHK(dev_malloc(&c->d_partials, sizeof(double) * oa::NSUMS_PLANE * oa::PLANE_MAX_BLOCKS));
    if (!c->d_sums) HIPCHK(dev_malloc(&c->d_sums, sizeof(double) * oa::NSUMS_PLANE));
    if (!c->d_solve) HIPCHK(dev_malloc(&c->d_solve, sizeof(double) * 32));
    if (!c->h_poll) {
        HIPCHK(hipHostMalloc((void **)&c->h_poll, 8 * sizeof(int32_t), hipHostMallocMapped));
        for (int k = 0; k < 8; ++k) c->h_poll[k] = 0;
    }
    if (!c->h_state_pin) HIPCHK(hipHostMalloc((void **)&c->h_state_pin, sizeof(oa::DevState), hipHostMallocDefault));
    return OA_OK;
}

// small device -> host read-back through a pinned scratch buffer, then a stream sync (a pageable destination costs
// ~30 us per copy; uploads do half a dozen of these)
// Small per-workgroup results (bounding-box partials, block maxima, counts) that the HOST reduces: the kernel stores them
// straight into pinned, device-mapped host memory, the host waits for the stream and reads -- no device buffer, no copy
// operation (an upload is bound by its number of enqueued operations, ~5 us each, and every read-back was two).
// result_ptr: where the kernel writes (device view) / where the host reads (host view); nullptr when `bytes` do not fit.
constexpr size_t RESULT_BYTES = 1 << 16;
int result_buffer(oa_ctx *c, size_t bytes, void **dev_view, const void **host_view)
{
    *dev_view = nullptr; *host_view = nullptr;
    if (bytes > RESULT_BYTES || !c->tune.mapped_results) return OA_OK;
    if (!c->h_result) {
        HIPCHK(hipHostMalloc((void **)&c->h_result, RESULT_BYTES, hipHostMallocMapped));
        void *dp = nullptr;
        if (hipHostGetDevicePointer(&dp, c->h_result, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(c->h_result); c->h_result = nullptr; return OA_OK; }
        c->d_result_view = dp;
    }
    *dev_view = c->d_result_view; *host_view = c->h_result;
    return OA_OK;
}

int read_small(oa_ctx *c, void *dst, const void *d_src, size_t bytes)
{
    constexpr size_t SCRATCH = 1 << 16;
    if (!c->h_scratch) HIPCHK(hipHostMalloc((void **)&c->h_scratch, SCRATCH, hipHostMallocDefault));
    if (bytes <= SCRATCH) {
        HIPCHK(hipMemcpyAsync(c->h_scratch, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        memcpy(dst, c->h_scratch, bytes);
    } else {
        HIPCHK(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return OA_OK;
}

int ensure_history(oa_ctx *c, int n)
{
    n = std::max(16, std::min(n, 1 << 16));
    if (n <= c->max_records) return OA_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->h_hist_map) { (void)hipHostFree(c->h_hist_map); c->h_hist_map = nullptr; c->d_hist = nullptr; }
    HIPCHK(hipHostMalloc((void **)&c->h_hist_map, sizeof(oa::StepRecord) * (size_t)n, hipHostMallocMapped));
    void *dp = nullptr;
    HIPCHK(hipHostGetDevicePointer(&dp, c->h_hist_map, 0));
    c->d_hist = (oa::StepRecord *)dp;
    c->max_records = n;
    return OA_OK;
}

int ensure_events(oa_ctx *c, int n_pairs)
{
    while ((int)c->ev.size() < 2 * n_pairs) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        c->ev.push_back(e);
    }
    if (!c->ev_loop0) { HIPCHK(hipEventCreate(&c->ev_loop0)); HIPCHK(hipEventCreate(&c->ev_loop1)); }
    return OA_OK;
}

int check_ready(oa_ctx *c)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (c->tgt.nt <= 0 || !c->tgt.d_tg) return fail(OA_E_STATE, "target not set (oa_set_target)");
    if (!c->src.d_src4) return fail(OA_E_STATE, "source not set (oa_set_source)");
    if (!c->have_mats) return fail(OA_E_STATE, "matrices not set (oa_set_matrices)");
    return OA_OK;
}

// every query through the tree: on request, and in auto mode for shards of up to `auto_max` points -- one wave per
// query has far lower latency than the one-thread-per-query grid kernels until the waves no longer fit the chip
// (measured crossover after the round-2 grid kernels: 3e3 .. 1.4e4 points for vertices -- the grid kernel spreads a
// query over 2 or 4 lanes when the shard is small --, 1.5e4 .. 2e4 for triangles, later for big targets whose grid no
// longer sits in cache; profiles/r02l_search_mode_crossover.txt.  Round 1: 1.2e4 .. 2.4e4 and 2.8e4 .. 4e4.)
inline int vertex_tree_max(const oa_ctx *c) { return c->tgt.nt >= 500000 ? 14336 : 3072; }
inline int tri_tree_max(const oa_ctx *c) { return c->tgt.n_tris >= 1000000 ? 20480 : (c->tgt.n_tris >= 250000 ? 18432 : 15360); }
// ... and while the pose still moves by a good part of a cell per iteration (stale seeds, long reach: the first
// iterations of a run, i.e. ALL of a typical early-exit run) the tree wins up to much larger shards (5-iteration runs
// from a cold start, profiles/r02l_search_mode_crossover_short_runs.txt): shards between the two limits get both
// searches enqueued and DevState::tree_turn decides on the device
inline int vertex_tree_early(const oa_ctx *c) { return c->tgt.nt >= 500000 ? 28672 : 8192; }
inline int tri_tree_early(const oa_ctx *c) { return c->tgt.n_tris >= 1000000 ? 57344 : (c->tgt.n_tris >= 250000 ? 40960 : 22528); }
inline bool bvh_whole(const oa_ctx *c, bool ok, int auto_max)
{
    if (!ok) return false;
    return c->grid_mode == 2 || (c->grid_mode == -1 && c->src.ns <= auto_max);
}
int build_grid(oa_ctx *c);
int build_safe_radii(oa_ctx *c);
// Stable argsort of keys of `bits` bits (30: Morton keys) on the context's stream, no wait: order = the indices in the keys' stable
// ascending order.  The library's own sorts (oa_sort.hpp): one workgroup up to SORT_SMALL_MAX keys, the LSD argsort above that, at
// most oa::SORT_MAX_N keys.
int sort_order_bits(oa_ctx *c, const unsigned *keys, int *order, size_t n, int bits)
{
    DevTmp<char> tmp;
    if (n > (size_t)oa::SORT_SMALL_MAX) HIPCHK(tmp.alloc(oa::sort_order_tmp_bytes(n)));
    HIPCHK(oa::sort_order((void *)tmp.p, keys, order, n, bits, c->stream));
    return OA_OK;
}
// keys[0 .. n) (non-negative ints below 2^bits) -> sorted[] ascending and order[] = where each came from (stable)
int sort_ints(oa_ctx *c, const int *keys, int *sorted, int *order, size_t n, int bits)
{
    int rc = sort_order_bits(c, (const unsigned *)keys, order, n, bits);
    if (rc || n == 0) return rc;
    hipLaunchKernelGGL(oa::k_gather_int, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, keys, (const int *)order, (int)n, sorted);
    HIPCHK(hipGetLastError());
    return OA_OK;
}
// one more, more significant key on top of an order (oa_sort.hpp, lex_order_next): order = by keys, equal keys as prev has them.  The
// keys are overwritten.  On the context's stream, no wait.
int lex_order_next(oa_ctx *c, unsigned *keys, int bits, const int *prev, int *order, size_t n)
{
    DevTmp<char> tmp;
    HIPCHK(tmp.alloc(oa::lex_order_tmp_bytes(n)));
    HIPCHK(oa::lex_order_next((void *)tmp.p, keys, bits, prev, order, n, c->stream));
    return OA_OK;
}
inline int bits_for(long long n_values) { int b = 1; while (b < 32 && (1ll << b) < n_values) ++b; return b; }
constexpr long long SAFE_LAZY_ITERS = 8;   // OA_GRID_SAFE=1: loop iterations a target has to see before its safe radii are built
// OA_GRID_SAFE=1: the radii are built once the target has seen SAFE_LAZY_ITERS iterations of a loop (counted once per iteration,
// launch_search_accumulate).  The array is allocated with the grid; the build is ONE launch on the context's stream and no
// allocation -- so it may sit between two iterations of a running loop, on the caller's stream or a multi-device child's
// (round 4 allocated here: inside a group's loop an allocation can wait for another child's stream, whose gather kernel waits
// for the post this thread has not enqueued yet -- children therefore built between loops only).
int safe_radii_lazy(oa_ctx *c)
{
    if (c->tune.grid_safe != 1 || c->tgt.safe_ok || !c->tgt.d_safe_by_idx) return OA_OK;
    return c->tgt.target_iters > SAFE_LAZY_ITERS ? build_safe_radii(c) : OA_OK;
}
int build_sorted_images(oa_ctx *c);
int build_tri_grid(oa_ctx *c, const double *diag_sum_known = nullptr);
int build_tri_ring(oa_ctx *c);
int build_tri_fine(oa_ctx *c);
// OA_TRI_RING=1: the neighbour lists are built once the mesh has served TRI_RING_LAZY_ITERS searches of a loop -- while the pose
// still moves by a good part of a triangle no query is within its seed's accept radius, and a short early-exit call should not
// pay for the build.  The buffer is allocated with the grid (never inside a loop: an allocation can wait for another stream,
// see safe_radii_lazy); the build itself is one launch on the context's stream, the searches queue behind it.
constexpr long long TRI_RING_LAZY_ITERS = 4;
int tri_ring_lazy(oa_ctx *c, bool counting)
{
    if (c->tune.tri_ring != 1 || c->tgt.tri_ring_ok || !c->tgt.d_tri_ring) return OA_OK;
    if (counting) ++c->tgt.tri_iters;
    return c->tgt.tri_iters > TRI_RING_LAZY_ITERS ? build_tri_ring(c) : OA_OK;
}
int build_bvh(oa_ctx *c, bool tri);
int ensure_boundary(oa_ctx *c, int k, double angle_deg);
int build_bvh_arrays(oa_ctx *c, bool tri, const float *d_xyz, int stride, int n, const double frame_lo[3], const double frame_hi[3],
                     oa::BvhParams &bp, DevBuf<float4> &d_box, DevBuf<float4> &d_prims, bool &ok);
int scan_counts(oa_ctx *c, const int *d_counts, int n, long long *d_off, DevTmp<char> &tmp);

// one wave per query: 4 queries per workgroup, workgroups loop when there are more queries than that
inline unsigned bvh_blocks(const oa_ctx *c, bool listed, bool acc = false)
{
    const int items = listed ? std::min(c->src.ns, 1 << 17) : c->src.ns;
    if (acc) return (unsigned)std::max(1, std::min((items + 15) / 16, c->n_cu * 4));   // workgroups of 16 waves
    return (unsigned)std::max(1, std::min((items + 3) / 4, c->n_cu * (listed ? c->tune.list_blocks_per_cu : 16)));   // 16 waves per SIMD: enough to fill the chip, cheap to dispatch when the list is empty
}

oa::NormalTest normal_test(const oa_ctx *c)
{
    oa::NormalTest nrm{};
    if (c->normals_on) { nrm.src_n = c->src.d_src_n; nrm.tgt_n = c->tgt.surface ? nullptr : c->tgt.d_tgt_n; nrm.cos_min = c->cos_min; }
    return nrm;
}

// what pair_fetch's callers behind a search pass on: the normal-angle test and, RECIP (oa_set_reciprocal on), k_recip_check's verdict
template <bool RECIP>
oa::PairTest<RECIP> pair_test(const oa_ctx *c)
{
    oa::PairTest<RECIP> nrm{};
    static_cast<oa::NormalTest &>(nrm) = normal_test(c);
    if constexpr (RECIP) nrm.recip_ok = c->src.d_recip_ok;
    return nrm;
}

// the target normals of a cloud (a surface target takes its triangles' geometric normals: null)
inline const float *plane_tn(const oa_ctx *c) { return c->tgt.surface ? (const float *)nullptr : (const float *)c->tgt.d_tgt_n; }

// One launch of a kernel that opens with pair_fetch and only reads the pairs (the filters' stages, k_residual_keys): its leading
// arguments, as launch_accumulate_as's lambda holds the writing kernels'; each caller adds its own behind the test
template <class Kern, class Test, class... Tail>
void launch_pair_reader(oa_ctx *c, Kern *kern, unsigned blocks, unsigned threads, const Test &nrm, const Tail &... tail)
{
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, c->stream, (const oa::DevState *)c->d_state, (const float4 *)c->src.d_src4, c->src.ns,
                       (const float *)c->tgt.d_tgt_xyz, (const unsigned long long *)c->src.d_keys,
                       c->tgt.surface ? (const float4 *)nullptr : (const float4 *)c->src.d_win, c->tgt.surface ? (const float4 *)c->tgt.d_tri9 : (const float4 *)nullptr,
                       nrm, tail...);
}

// ------------------------------------------------------------------------------------------------
// The pair filters, between the search and the accumulation: the reciprocal check (oa_set_reciprocal, oa_recip.hpp),
// the boundary rejection (oa_set_reject_boundary, oa_boundary.hpp) and the trim (oa_set_trim, oa_trim.hpp).  Each leaves its
// verdict in src.d_recip_ok, one byte per slot, and a step with any of them on accumulates through the RECIP kernels.  What every
// caller needs of the three is said once each: on? (verdict_on), the refusals (refuse_filters_shard, refuse_filters_multi), what
// a step needs before its loop (ensure_filters), the counters back to zero (filters_clear), and the stages of a step in their
// order (launch_filters, behind launch_trim).  A new filter is added to these and to nothing else.
// ------------------------------------------------------------------------------------------------
inline bool trim_on(const oa_ctx *c) { return c->trim_fraction != 0.0; }
inline bool trim_auto(const oa_ctx *c) { return c->trim_fraction < 0.0; }
inline bool verdict_on(const oa_ctx *c) { return c->recip_on || trim_on(c) || c->bnd_on; }

// The step counters of the filters in `which` back to zero (those that exist), and the host waits: whatever stream the next step
// runs on finds them cleared.  Called with no step in flight (a new source, a changed setting, the allocation): the
// OA_STAT_*_REJECTED and OA_STAT_TRIM_* figures never speak of an older one
enum : unsigned { FILTER_RECIP = 1u, FILTER_BND = 2u, FILTER_TRIM = 4u, FILTER_ALL = 7u };
int filters_clear(oa_ctx *c, unsigned which = FILTER_ALL)
{
    auto clear = [&](void *d_block, size_t bytes) -> int {
        if (!d_block) return OA_OK;
        HIPCHK(hipMemsetAsync(d_block, 0, bytes, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return OA_OK;
    };
    int rc = OA_OK;
    if (which & FILTER_RECIP) rc = clear(c->d_recip_count, sizeof(unsigned) * oa::RECIP_COUNT_WORDS);
    if (!rc && (which & FILTER_BND)) rc = clear(c->d_bnd_count, sizeof(unsigned) * oa::BND_COUNT_WORDS);
    if (!rc && (which & FILTER_TRIM)) rc = clear(c->d_trim, sizeof(oa::DevTrim));     // (the last step's figures and the running counters)
    return rc;
}

// `who` on a context that holds a shard.  The reciprocal check needs every selected source point, and the trim's cut is an order
// statistic of the world's residuals: a shard cannot see the other shards'.  The target is replicated, so a shard could answer
// the boundary question for itself -- but the verdict byte's path has never run in shards.
// The order is reciprocal, trim, boundary -- not the stages' order: with the trim and the boundary both on, the error names oa_set_trim
int refuse_filters_shard(const oa_ctx *c, const char *who)
{
    if (!verdict_on(c) || !(c->parent || c->src_shards > 1)) return OA_OK;
    if (c->recip_on)
        return fail(OA_E_STATE, "%s with the reciprocal check on needs the whole selection on one context: this one holds a shard (upload shard 0 of 1, or call oa_set_reciprocal(ctx, 0, 1))", who);
    if (trim_on(c))
        return fail(OA_E_STATE, "%s with oa_set_trim on needs the whole selection on one context: this one holds a shard (upload shard 0 of 1, or call oa_set_trim(ctx, 0, 0, 2))", who);
    return fail(OA_E_STATE, "%s with oa_set_reject_boundary on needs the whole selection on one context: this one holds a shard (upload shard 0 of 1, or call oa_set_reject_boundary(ctx, 0, 16, 90))", who);
}

// ... and `who` on a multi-device context, or in the split-phase loop (refuse_wide_row): in the same order
int refuse_filters_multi(const oa_ctx *c, const char *who)
{
    if (c->recip_on)
        return fail(OA_E_STATE, "%s: the reciprocal check needs every selected source point on one device: it runs on a single-device context through oa_run / oa_iterate / oa_make_pairs (call oa_set_reciprocal(ctx, 0, 1) for this path)", who);
    if (trim_on(c))
        return fail(OA_E_STATE, "%s: oa_set_trim needs every selected source point's residual on one device: it runs on a single-device context through oa_run / oa_iterate / oa_make_pairs (call oa_set_trim(ctx, 0, 0, 2) for this path)", who);
    if (c->bnd_on)
        return fail(OA_E_STATE, "%s: oa_set_reject_boundary runs on a single-device context through oa_run / oa_iterate / oa_make_pairs (call oa_set_reject_boundary(ctx, 0, 16, 90) for this path)", who);
    return OA_OK;
}

// oa_set_reciprocal: what a step with the check on needs, before its loop starts (allocations, and the tree build waits for the
// stream): the counters, and -- once per oa_set_source -- the box tree over the selected source points in align-local space,
// inside the box of their finite coordinates.  The pose never enters: oa_set_matrices does not touch it.
int ensure_recip(oa_ctx *c)
{
    if (!c->recip_on) return OA_OK;
    if (!c->d_recip_count) {                                        // (whatever ns is: an empty selection still reads the stat)
        HIPCHK(dev_malloc(&c->d_recip_count, sizeof(unsigned) * oa::RECIP_COUNT_WORDS));
        const int rcc = filters_clear(c, FILTER_RECIP);
        if (rcc) return rcc;
    }
    if (c->src.ns <= 0 || c->src.sbvh_ok) return OA_OK;                 // (an empty selection: no slot, no tree -- and no launch)
    c->src.d_sbvh_box.reset(); c->src.d_sbvh_prims.reset();
    const int nb = oa::RECIP_FRAME_BLOCKS;
    DevTmp<float> d_bb;
    HIPCHK(d_bb.alloc(6 * (size_t)nb));
    hipLaunchKernelGGL(oa::k_recip_frame, dim3(nb), dim3(256), 0, c->stream, (const float4 *)c->src.d_src4, c->src.ns, d_bb.p);
    HIPCHK(hipGetLastError());
    std::vector<float> bb(6 * (size_t)nb);
    int rc = read_small(c, bb.data(), d_bb.p, sizeof(float) * bb.size());
    if (rc) return rc;
    float l[3] = { INFINITY, INFINITY, INFINITY }, h[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int b = 0; b < nb; ++b)
        for (int a = 0; a < 3; ++a) { l[a] = std::min(l[a], bb[6 * (size_t)b + a]); h[a] = std::max(h[a], bb[6 * (size_t)b + 3 + a]); }
    double lo[3] = { 0.0, 0.0, 0.0 }, hi[3] = { 0.0, 0.0, 0.0 };
    for (int a = 0; a < 3; ++a) if (l[a] <= h[a]) { lo[a] = l[a]; hi[a] = h[a]; }     // (no finite coordinate: any frame will do)
    bool ok = false;
    if ((rc = build_bvh_arrays(c, false, (const float *)c->src.d_src4, 4, c->src.ns, lo, hi, c->src.sbvh, c->src.d_sbvh_box, c->src.d_sbvh_prims, ok))) return rc;
    if (!ok) return fail(OA_E_CAPACITY, "oa_set_reciprocal: the source's box tree would need more than %d levels", oa::BVH_MAX_LEVELS);
    c->src.sbvh_ok = true;
    return OA_OK;
}

// the reciprocal check's stage: one wave per slot, every verdict byte and the step's count.
// metric_n: the pair_fetch<.., METRIC_N> of the accumulation that follows (the plane and GICP metrics; never the emitting one)
int launch_recip(oa_ctx *c, bool metric_n)
{
    auto *kern = metric_n ? oa::k_recip_check<true> : oa::k_recip_check<false>;
    const unsigned blocks = (unsigned)std::max(1, std::min((c->src.ns + oa::RECIP_WPB - 1) / oa::RECIP_WPB, c->n_cu * 16));
    // (the test without the verdict: this launch forms it)
    launch_pair_reader(c, kern, blocks, (unsigned)(oa::RECIP_WPB * 64), normal_test(c), plane_tn(c), c->src.sbvh, (const float4 *)c->src.d_sbvh_box,
                       (const float4 *)c->src.d_sbvh_prims, (float)(c->recip_ratio * c->recip_ratio), (unsigned char *)c->src.d_recip_ok, (unsigned *)c->d_recip_count);
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// oa_set_reject_boundary: what a step with the setting on needs, before its loop starts: the counters and the target's masks
int ensure_bnd_step(oa_ctx *c)
{
    if (!c->bnd_on) return OA_OK;
    if (!c->d_bnd_count) {
        HIPCHK(dev_malloc(&c->d_bnd_count, sizeof(unsigned) * oa::BND_COUNT_WORDS));
        const int rcc = filters_clear(c, FILTER_BND);
        if (rcc) return rcc;
    }
    return ensure_boundary(c, c->bnd_k, c->bnd_angle);
}

// the boundary rejection's stage: byte 0 for every pair on the target's boundary
int launch_boundary(oa_ctx *c)
{
    const unsigned blocks = (unsigned)std::max(1, std::min((c->src.ns + oa::BND_VERDICT_THREADS - 1) / oa::BND_VERDICT_THREADS, c->n_cu * 2));
    launch_pair_reader(c, oa::k_boundary_verdict, blocks, (unsigned)oa::BND_VERDICT_THREADS, normal_test(c), (const int *)c->tgt.d_tris,
                       (const unsigned char *)c->tgt.d_bnd_emask, (const unsigned char *)c->tgt.d_bnd_vmask, (unsigned char *)c->src.d_recip_ok, (unsigned *)c->d_bnd_count);
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// oa_set_trim: what a step with the trim on needs, before its loop starts: the keys, the trim's state with the setting in it, and
// the buffers of the mode in force -- never allocated inside the loop
int ensure_trim(oa_ctx *c)
{
    if (!trim_on(c)) return OA_OK;
    if (trim_auto(c) && (long long)c->src.ns > oa::TRIM_AUTO_MAX)
        return fail(OA_E_CAPACITY, "oa_set_trim: the estimated share takes up to %lld points (this selection: %d)", oa::TRIM_AUTO_MAX, c->src.ns);
    if (!c->d_trim) {
        HIPCHK(dev_malloc(&c->d_trim, sizeof(oa::DevTrim)));
        const int rcc = filters_clear(c, FILTER_TRIM);
        if (rcc) return rcc;
    }
    {   // the setting: everything in front of the counters (the stream is idle or about to be waited for; the figures stay)
        oa::DevTrim h{};
        h.sel.p = trim_auto(c) ? 0.0 : c->trim_fraction;
        h.sel.k_min = 3u;
        h.lambda = c->trim_lambda;
        h.fraction_min = c->trim_min;
        HIPCHK(hipMemcpyAsync(c->d_trim, &h, offsetof(oa::DevTrim, running), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (c->src.ns <= 0) return OA_OK;                                   // an empty selection: no slot, no launch
    const size_t ns = (size_t)c->src.ns;
    if (!c->src.d_rkeys) HIPCHK(dev_malloc(&c->src.d_rkeys, sizeof(uint32_t) * ns));
    if (!c->d_trim_hist) HIPCHK(dev_malloc(&c->d_trim_hist, sizeof(uint32_t) * oa::SEL_LEVELS * oa::SEL_BINS));
    if (trim_auto(c)) {
        const size_t n_tiles = (size_t)oa::trim_tiles(c->src.ns);
        if (!c->src.d_trim_sorted) HIPCHK(dev_malloc(&c->src.d_trim_sorted, sizeof(uint32_t) * ns));
        if (!c->src.d_trim_order) HIPCHK(dev_malloc(&c->src.d_trim_order, sizeof(int) * ns));
        if (!c->src.d_trim_tmp && ns > (size_t)oa::SORT_SMALL_MAX) HIPCHK(dev_malloc(&c->src.d_trim_tmp, oa::sort_order_tmp_bytes(ns)));
        if (!c->src.d_trim_tiles) HIPCHK(dev_malloc(&c->src.d_trim_tiles, sizeof(double) * n_tiles));
        if (!c->src.d_trim_min) HIPCHK(dev_malloc(&c->src.d_trim_min, sizeof(oa::TrimTileMin) * n_tiles));
    }
    return OA_OK;
}

// What a step needs of the filters that are on, before its loop starts and never inside it: the verdict bytes (allocated here and
// nowhere else; an empty selection has no slot and gets none), then each filter's own -- the source tree, the trim's state, the
// target's masks, all on this stream
int ensure_filters(oa_ctx *c)
{
    int rc;
    if (verdict_on(c) && c->src.ns > 0 && !c->src.d_recip_ok) HIPCHK(dev_malloc(&c->src.d_recip_ok, (size_t)c->src.ns));
    if ((rc = ensure_recip(c))) return rc;
    if ((rc = ensure_trim(c))) return rc;
    return ensure_bnd_step(c);
}

// acc: a whole-shard search of the loop that also takes the pair test and the sums (k_bvh_search<TRI, true>)
template <bool TRI>
int launch_bvh(oa_ctx *c, const int *list, const int *list_count, int turn = -1, bool acc = false)
{
    const unsigned blocks = bvh_blocks(c, list != nullptr, acc);
    // whole-shard vertex searches take seeds on their safe radii (docs/HISTORY.md 4.4 / 4.8): both arrays or neither
    const float *safe_by_idx = nullptr;
    uint2 *wsafe = nullptr;
    if (!TRI && !list && c->tune.grid_safe) {
        if (acc) { const int rcs = safe_radii_lazy(c); if (rcs) return rcs; }
        if (c->tgt.safe_ok && c->tgt.d_safe_by_idx && c->src.d_wsafe) { safe_by_idx = c->tgt.d_safe_by_idx; wsafe = c->src.d_wsafe; }
    }
    auto launch = [&](auto ACC, unsigned threads, const oa::NormalTest &nrm, double *partials) {
        hipLaunchKernelGGL((oa::k_bvh_search<TRI, decltype(ACC)::value>), dim3(blocks), dim3(threads), 0, c->stream, c->d_state, c->src.d_src4, c->src.ns, TRI ? c->tgt.tbvh : c->tgt.bvh,
                           TRI ? c->tgt.d_tbvh_box : c->tgt.d_bvh_box, TRI ? c->tgt.d_tbvh_prims : c->tgt.d_bvh_prims, c->tgt.d_tri9, c->src.d_prev, TRI ? (float4 *)nullptr : c->src.d_win, c->src.d_keys,
                           list, list_count, turn, nrm, partials, safe_by_idx, wsafe);
    };
    if (acc) launch(std::true_type{}, 1024, normal_test(c), c->d_partials);
    else launch(std::false_type{}, 256, oa::NormalTest{}, nullptr);
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// lanes per query of the vertex grid search: shards too small to fill the chip's wave slots split every query's rows
// between 2 or 4 lanes.  Measured on 256 CUs with the round-2 kernel (profiles/r02n_grid_lanes_sweep.txt; round 1:
// r01h_grid_lanes_sweep.txt): against a target that sits in cache 4 lanes win up to ~20k queries and 2 up to ~350k;
// against >= 500k vertices every round trip is longer and the lanes pay for longer: 4 up to ~100k queries, 2 up to
// ~700k; 1M queries lose 7 % with 2
inline int grid_lanes_for(const oa_ctx *c)
{
    int lanes = c->tune.grid_lanes;
    if (lanes != 1 && lanes != 2 && lanes != 4) {
        const bool big = c->tgt.nt >= 500000;
        lanes = (c->src.ns <= (big ? 400 : 80) * c->n_cu) ? 4 : ((c->src.ns <= (big ? 2800 : 1400) * c->n_cu) ? 2 : 1);
    }
    return lanes;
}

// lanes per query of the triangle grid search, as for the vertex grid (measured on 256 CUs with the round-2 kernel,
// profiles/r02n_grid_lanes_sweep.txt: small meshes 4 lanes up to ~32k queries, 2 up to ~180k; >= 250k triangles
// 4 up to ~100k, 2 up to ~800k)
inline int tri_lanes_for(const oa_ctx *c)
{
    int lanes = c->tune.grid_lanes;
    if (lanes != 1 && lanes != 2 && lanes != 4) {
        const bool big = c->tgt.n_tris >= 250000;
        lanes = (c->src.ns <= (big ? 400 : 128) * c->n_cu) ? 4 : ((c->src.ns <= (big ? 3200 : 700) * c->n_cu) ? 2 : 1);
    }
    return lanes;
}

// Workgroups of the canonical accumulation (k_pair_accumulate_canon, and the epilogue of k_nn_search_grid<L, true>): one
// thread per (slot, lane of the query).  0 = the shard is too large for it (> ACC_MAX_BLOCKS rows before combining) or the
// target is a surface: the grid-stride k_pair_accumulate is used instead.
// (512 threads per workgroup from 262k (query, lane) pairs on: half the rows for the reduction behind it; below that the
//  finer workgroups balance better)
// (surface targets, round 4: the triangle grid search accumulates in its epilogue too -- k_tri_search_grid<L, .., ACC> --, always
//  in workgroups of 256 threads, with ITS lanes per query)
inline int canon_lanes(const oa_ctx *c) { return c->tgt.surface ? tri_lanes_for(c) : grid_lanes_for(c); }
inline int canon_threads(const oa_ctx *c)
{
    if (c->tgt.surface) return 256;
    if (c->tune.acc_threads == 256 || c->tune.acc_threads == 512) return c->tune.acc_threads;   // OA_ACC_THREADS (A/B)
    return (long long)c->src.ns * grid_lanes_for(c) >= 262144 ? 512 : 256;
}
inline int canon_blocks(const oa_ctx *c)
{
    if (c->src.ns <= 0 || (c->tgt.surface && !c->tune.tri_canon)) return 0;
    const int t = canon_threads(c);
    const long long b = ((long long)c->src.ns * canon_lanes(c) + t - 1) / t;
    return b <= oa::ACC_MAX_BLOCKS ? (int)b : 0;
}

// A run-time value as a compile-time constant out of a closed list: f(std::integral_constant<int, V>{}) for the V among Others that
// equals v, for Fallback when none does.  The list at a call site is what that site can launch; for the kernel templates of the
// family units it has to stay within oa_families.hpp's list for the flavour (the linker says so when it does not).
template <int Fallback, int... Others, typename F>
inline void dispatch(int v, F &&f)
{
    const bool hit = ((v == Others ? (f(std::integral_constant<int, Others>{}), true) : false) || ...);
    if (!hit) f(std::integral_constant<int, Fallback>{});
}
template <int V> using int_c = std::integral_constant<int, V>;
constexpr std::true_type yes{};
constexpr std::false_type no{};

enum BruteKernel { BRUTE_PLAIN = 0, BRUTE_FILTERED = 1, BRUTE_MFMA = 2, BRUTE_SORTED = 3 };   // brute force over vertices (the values are OA_STAT_BRUTE_KERNEL's)
BruteKernel brute_kernel(const oa_ctx *c)
{
    if (!c->tgt.filter_ok || !c->tune.nn_filter) return BRUTE_PLAIN;
#if defined(OA_EXPERIMENTS)
    if (c->tune.nn_mfma && c->tgt.d_tfm && c->src.R == 4 && c->tile_groups == oa::FTILE_GROUPS) return BRUTE_MFMA;
    if (!(c->tune.nn_sort && c->tgt.d_tfs)) return BRUTE_FILTERED;
#endif
    return (c->tune.nn_sort && c->tgt.d_tfs) ? BRUTE_SORTED : BRUTE_PLAIN;
}

// What the next search launch looks like: which search (loop and one-shot calls alike), and the loop's fusion plan.
//   TREE   every query through the tree, which also accumulates (k_bvh_search<.., true>)
//   DUAL   tree and grid both enqueued, DevState::tree_turn picks on the device; both accumulate; the grid search finishes
//          its leftovers itself (it only has the turn once the pose has settled)
//   GRID   the grid search.  FAST: it finishes its leftovers itself and accumulates -- two launches per iteration.  SAFE:
//          grid search -> tree search of the hand-over list -> k_pair_accumulate_canon -- four launches, and the right
//          thing when many queries are handed over (one wave per query over the whole chip instead of the owner wave
//          walking its own leftovers one after the other: a cold start far from the target is 3-4x slower the FAST way).
//          Both leave bitwise the same rows, so the choice -- taken per iteration from what the host last heard about the
//          hand-over list, i.e. timing dependent -- never shows in a result.
//   PLAIN  search, then accumulate (brute force; surface grid; shards too large for the canonical rows)
enum SearchPlan { PLAN_PLAIN, PLAN_TREE, PLAN_DUAL, PLAN_GRID };
enum SearchKind { SEARCH_TREE, SEARCH_GRID, SEARCH_BRUTE };        // whole-shard tree | vertex / triangle grid, leftovers through the tree | SearchChoice::brute / k_tri_search_all
struct SearchChoice {
    SearchKind kind = SEARCH_BRUTE;
    BruteKernel brute = BRUTE_PLAIN;
    bool dual = false;              // SEARCH_GRID: tree and grid take turns (DevState::tree_turn)
    int lanes = 1;                  // SEARCH_GRID: lanes per query
    // triangle grid, experiments: a front search settles what it can and lists the rest; not while tree and grid take turns
    bool settle_front = false;      // k_tri_settle (the settled-pose search, oa_tri_fine.hpp)
    bool accept_front = false;      // k_tri_accept (seed + neighbour lists, oa_tri_ring.hpp), once the lists are built
    SearchPlan plan = PLAN_PLAIN;   // a loop with fused_acc only
};
// a loss or per-vertex weights are set: the loop's pairs carry weights (weighted kernels, the PLAIN plan)
inline bool weighted(const oa_ctx *c) { return c->loss != OA_LOSS_NONE || c->src.d_w != nullptr; }
// the metrics that sum the wide row (NSUMS_PLANE) and take the 6 x 6 solve: point-to-plane, plane-to-plane (GICP) and symmetric
inline bool plane_row_metric(const oa_ctx *c) { return c->metric == OA_METRIC_PLANE || c->metric == OA_METRIC_GICP || c->metric == OA_METRIC_SYMMETRIC; }
// ... by the name the error texts give them ("the %s metric"); null: the point metric
inline const char *normal_metric_noun(int metric)
{
    return metric == OA_METRIC_PLANE ? "plane" : metric == OA_METRIC_GICP ? "GICP" : metric == OA_METRIC_SYMMETRIC ? "symmetric" : nullptr;
}
// ... and the loss takes its scale from the step's own residuals (oa_set_robust_auto; inert without a loss)
inline bool auto_scale(const oa_ctx *c) { return c->loss != OA_LOSS_NONE && c->robust_p > 0.0; }

SearchChoice choose_search(const oa_ctx *c)
{
    SearchChoice s;
    s.brute = brute_kernel(c);
    // (the grid searches hand their leftovers to the tree; mode 2 never gets to the grid arm: the whole-shard tree took it, or tree_ok is false)
    const bool tree_ok = c->tgt.surface ? c->tgt.tbvh_ok : c->tgt.bvh_ok, grid_ok = c->tgt.surface ? c->tgt.tri_grid_ok : (c->tgt.grid_ok && c->tgt.filter_ok && c->tune.nn_filter);
    if (bvh_whole(c, tree_ok, c->tgt.surface ? tri_tree_max(c) : vertex_tree_max(c))) s.kind = SEARCH_TREE;
    else if (grid_ok && tree_ok && c->grid_mode != 0) {
        s.kind = SEARCH_GRID;
        s.dual = c->grid_mode == -1 && c->tune.search_turns && c->src.ns <= (c->tgt.surface ? tri_tree_early(c) : vertex_tree_early(c));
        s.lanes = c->tgt.surface ? tri_lanes_for(c) : grid_lanes_for(c);
        s.settle_front = c->tgt.surface && c->tgt.tri_fine_ok && c->seeded && !s.dual;
        s.accept_front = c->tgt.surface && c->tune.tri_split && c->seeded && !s.dual;
    }
    // (the plane, GICP and symmetric metrics have no accumulating search epilogue: search, then k_pair_accumulate_plane / _gicp / _symm -- as with
    //  fused_acc off; nor does a weighted step: no search epilogue knows about weights -- nor about the reciprocal check or the trim)
    if (!c->tune.fused_acc || !c->loop_active || c->src.ns <= 0 || plane_row_metric(c) || weighted(c) || verdict_on(c)) return s;
    // (the accumulating tree search needs twice the registers of the plain one: worth it while the shard is small enough
    //  that occupancy does not matter -- 12k queries against 1M vertices: 58 us fused, 47 us search + accumulate)
    if (s.kind == SEARCH_TREE) s.plan = c->src.ns <= c->tune.tree_acc_max ? PLAN_TREE : PLAN_PLAIN;
    else if (s.kind != SEARCH_GRID || canon_blocks(c) == 0) s.plan = PLAN_PLAIN;
    else if (!c->tgt.surface) s.plan = s.dual ? PLAN_DUAL : PLAN_GRID;
    // the triangle grid search with the accumulating epilogue: shards above the zone where tree and grid take turns, and no
    // front search (k_tri_accept / k_tri_settle + the search of what they leave, which has no accumulating form)
    else s.plan = (!s.dual && !(s.accept_front && c->tgt.tri_ring_ok) && !s.settle_front && c->tune.tri_acc) ? PLAN_GRID : PLAN_PLAIN;
    return s;
}

// Does the enqueuing host wait for news from the device (h_poll) before each iteration of a loop?  With early exit on -- a
// halt it hears of saves the empty launches after it -- and on the adaptive grid path, which decides from recent news
bool loop_polls(const oa_ctx *c, const oa_settings *st)
{
    return c->h_poll && c->tune.run_poll && (st->early_exit || (choose_search(c).plan == PLAN_GRID && c->tune.grid_path == 0));
}

// PLAN_GRID: may this iteration's grid search finish its own leftovers?  Yes while the most any one wave handed over in
// the last iteration the host heard of is small (a wave walks its leftovers one after the other, ~5-10 us each).  The
// host stays within a few iterations of the device (oa_run throttles itself), so "last heard of" is recent; with no
// news from this loop yet the previous decision stands, and a loop starts SAFE unless it continues on warm seeds.
constexpr int FAST_WAVE_MAX = 3;
bool grid_fast_now(oa_ctx *c)
{
    if (c->tune.grid_path == 1) return true;
    if (c->tune.grid_path == 2) return false;
    bool fast = c->fast_prev;
    const volatile int32_t *poll = c->h_poll;
    const int n_done = poll ? poll[1] : 0;
    if (n_done > 0 && n_done >= c->iter_enq - 4) fast = poll[3] <= FAST_WAVE_MAX;
    else if (c->iter_enq == 0) fast = c->seeded && c->last_todo_wave_max >= 0 && c->last_todo_wave_max <= FAST_WAVE_MAX;
    else if (n_done <= 0 && c->iter_enq > 4) fast = false;          // the host ran far ahead of the device: no news, no risk
    if (c->tune.debug) fprintf(stderr, "[oa] grid path: iteration %d enqueued, device at %d, last hand-over %d entries / %d per wave (previous loop: %d) -> %s\n", c->iter_enq, n_done, poll ? poll[2] : -1, poll ? poll[3] : -1, c->last_todo_wave_max, fast ? "fast" : "safe");
    c->fast_prev = fast;
    return fast;
}

#if defined(OA_EXPERIMENTS)
// OA_GRID_STATS=1: launch(rows) enqueues an instrumented search that keeps one row of n_stat counters per wave (atomics on a dozen
// shared words slowed the launch 8x); h[0 .. n_stat) = the sums over the n_waves rows.  Synchronises.
template <typename Launch>
int wave_stats(oa_ctx *c, int n_stat, size_t n_waves, unsigned long long *h, Launch &&launch)
{
    std::vector<unsigned long long> rows((size_t)n_stat * n_waves);
    DevTmp<unsigned long long> d_rows;
    HIPCHK(d_rows.alloc(rows.size()));
    HIPCHK(hipMemsetAsync(d_rows, 0, sizeof(unsigned long long) * rows.size(), c->stream));
    launch(d_rows.p);
    HIPCHK(hipGetLastError());
    { int rcr = read_small(c, rows.data(), d_rows, sizeof(unsigned long long) * rows.size()); if (rcr) return rcr; }
    std::fill(h, h + n_stat, 0ull);
    for (size_t w = 0; w < n_waves; ++w) for (int k = 0; k < n_stat; ++k) h[k] += rows[w * (size_t)n_stat + (size_t)k];
    return OA_OK;
}
// the instrumented accumulating vertex grid search (one lane per query, 512 threads: 8 waves per workgroup): phase shares to stderr
template <typename Launch>
int vertex_grid_stats(oa_ctx *c, unsigned blocks, Launch &&launch)
{
    unsigned long long h[oa::GRID_STAT_N];
    { const int rcs = wave_stats(c, oa::GRID_STAT_N, (size_t)blocks * 8, h, launch); if (rcs) return rcs; }
    const double nw = (double)std::max(1ull, h[oa::GRID_STAT_WAVES]), ct = (double)std::max(1ull, h[oa::GRID_STAT_CYC_TOTAL]);
    fprintf(stderr, "[oa] vertex grid phases: %llu of %d queries settled by the seed's safe radius | per wave %.0f shader cycles, %.2f loop trips, %.2f scan trips, %.1f candidates per query (longest lane of a wave %.1f) | "
                    "prologue %.1f%% listing %.1f%% scan %.1f%% bookkeeping %.1f%% finish %.1f%% epilogue %.1f%% (loads + pair test %.1f%%, wave reduction %.1f%%, barrier %.1f%%)\n",
            h[oa::GRID_STAT_ACCEPTED], c->src.ns, ct / nw, h[oa::GRID_STAT_LOOP_TRIPS] / nw, h[oa::GRID_STAT_SCAN_TRIPS] / nw, h[oa::GRID_STAT_CANDIDATES] / (64.0 * nw),
            h[oa::GRID_STAT_MAX_LANE_CANDIDATES] / nw, 100.0 * h[oa::GRID_STAT_CYC_PROLOGUE] / ct, 100.0 * h[oa::GRID_STAT_CYC_LIST] / ct,
            100.0 * h[oa::GRID_STAT_CYC_SCAN] / ct, 100.0 * h[oa::GRID_STAT_CYC_BOOK] / ct, 100.0 * h[oa::GRID_STAT_CYC_FINISH] / ct,
            100.0 * h[oa::GRID_STAT_CYC_EPILOGUE] / ct, 100.0 * h[oa::GRID_STAT_CYC_EPI_PAIR] / ct, 100.0 * h[oa::GRID_STAT_CYC_EPI_REDUCE] / ct,
            100.0 * h[oa::GRID_STAT_CYC_EPI_BARRIER] / ct);
    return OA_OK;
}
#endif

// The grid search settles the queries near the target; the rest (far away, or in crowded cells) go through the tree: in the
// loop by the wave that owns them (acc), in one-shot calls through a list that k_bvh_search finishes.
int launch_vertex_grid(oa_ctx *c, const SearchChoice &s, bool acc)
{
    if (!acc && !c->loop_active) HIPCHK(hipMemsetAsync(c->src.d_todo_count, 0, 2 * sizeof(int), c->stream));
    if (s.dual) { int rcb = launch_bvh<false>(c, nullptr, nullptr, 1, acc); if (rcb) return rcb; }   // runs when DevState::tree_turn
    // {index, safe2} per slot beside the winner records: both or neither (OA_GRID_SAFE=0)
    if (acc) { const int rcs = safe_radii_lazy(c); if (rcs) return rcs; }
    const bool safe = c->tune.grid_safe && c->tgt.safe_ok && c->tgt.d_safe_by_idx && c->src.d_wsafe;
    // k_nn_search_grid<L, ACC, BT, STATS>; the accumulating form gets the tree, the pair test and the rows of partials
    auto launch = [&](auto L, auto ACC, auto BT, auto STATS, unsigned blocks, unsigned long long *stats) {
        constexpr bool A = decltype(ACC)::value;
        hipLaunchKernelGGL((oa::k_nn_search_grid<decltype(L)::value, A, decltype(BT)::value, decltype(STATS)::value>), dim3(blocks), dim3(decltype(BT)::value), 0, c->stream,
                           c->d_state, c->src.d_src4, c->src.ns, c->tgt.gp, c->tgt.d_cell_start, c->tgt.d_sorted, c->src.d_win, c->src.d_keys, c->src.d_todo_list, c->src.d_todo_count, s.dual ? 0 : -1,
                           A ? c->tgt.bvh : oa::BvhParams{}, A ? (const float4 *)c->tgt.d_bvh_box : nullptr, A ? (const float4 *)c->tgt.d_bvh_prims : nullptr,
                           A ? normal_test(c) : oa::NormalTest{}, A ? c->d_partials : nullptr, stats, safe ? c->tgt.d_safe_by_idx : nullptr, safe ? c->src.d_wsafe : nullptr);
    };
    if (!acc) {
        dispatch<1, 2, 4>(s.lanes, [&](auto L) { launch(L, no, int_c<256>{}, no, (unsigned)(((long long)c->src.ns * s.lanes + 255) / 256), nullptr); });
        HIPCHK(hipGetLastError());
        return launch_bvh<false>(c, c->src.d_todo_list, c->src.d_todo_count);
    }
    const unsigned ablocks = (unsigned)canon_blocks(c);
#if defined(OA_EXPERIMENTS)
    if (c->tune.grid_stats && s.lanes == 1 && canon_threads(c) == 512)
        return vertex_grid_stats(c, ablocks, [&](unsigned long long *stats) { launch(int_c<1>{}, yes, int_c<512>{}, yes, ablocks, stats); });
#endif
    dispatch<256, 512>(canon_threads(c), [&](auto BT) { dispatch<1, 2, 4>(s.lanes, [&](auto L) { launch(L, yes, BT, no, ablocks, nullptr); }); });
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// What k_nn_search_sorted reads beside the images (oa_kernels.hpp): the point records of k_sorted_point_setup for ns_pad slots, d_homes for
// `blocks` blocks of source points + the work queue's counters, both rewritten by k_sorted_block_homes.  They come with the source in
// brute-force mode (source_reset, oa_set_search_mode: never inside a loop, see safe_radii_lazy); the other modes get here at first use (a
// target without usable grid or tree), or should the blocks outgrow them.
int ensure_sorted_buffers(oa_ctx *c, int blocks)
{
    if (c->src.ns_pad > c->src.prec_cap) {
        c->src.d_prec.reset(); c->src.prec_cap = 0;
        HIPCHK(dev_malloc(&c->src.d_prec, sizeof(float4) * 4 * (size_t)c->src.ns_pad));   // (three float4 per slot + the lanes' point pairs)
        c->src.prec_cap = c->src.ns_pad;
    }
    if (blocks > c->src.homes_cap) {
        c->src.d_homes.reset(); c->src.homes_cap = 0;
        HIPCHK(dev_malloc(&c->src.d_homes, sizeof(int) * 2 * (size_t)blocks));
        c->src.homes_cap = blocks;
    }
    if (!c->src.d_qcnt) HIPCHK(dev_malloc(&c->src.d_qcnt, sizeof(int) * (size_t)(oa::SORTED_QUEUES * oa::SORTED_QUEUE_STRIDE)));
    return OA_OK;
}

// The sorted brute-force search: seed pass (the first search of a loop) -> point setup -> block homes -> search
int launch_brute_sorted(oa_ctx *c, const dim3 grid)
{
    // with seeds: one launch over n_splits_seeded splits.  Without (the first search of a loop): k_nn_seed_sorted -- every point
    // against the tile that holds its own slab --, then the whole search seeded from what that left in keys (OA_NN_HOME_PASS=0:
    // one unseeded launch over n_splits splits, as until r05z)
    const bool two = !c->win_seeds && c->tune.nn_home_pass && c->n_splits_seeded > 1;
    dim3 sgrid((unsigned)((c->win_seeds || two) ? c->n_splits_seeded : c->n_splits), grid.y);
    // long launches go through the work queue (oa_kernels.hpp): as many workgroups as the chip holds, the long items first
    const int q_splits = (int)sgrid.x, q_blocks = (int)sgrid.y;
    const long long q_wgs = (long long)c->n_cu * std::min(c->tune.nn_persist, c->src.R <= 4 ? 4 : 2);
    const bool queued = q_wgs > 0 && q_splits > 1 && (long long)q_splits * q_blocks >= (c->tune.nn_queue_min >= 0 ? (long long)c->tune.nn_queue_min : 4 * q_wgs);
    c->last_queue_wgs = queued ? (int)q_wgs : 0;
    { const int rcq = ensure_sorted_buffers(c, q_blocks); if (rcq) return rcq; }
    const int pass = two ? 2 : 0;                                   // (seeded from what the seed pass leaves in keys)
    if (two) {
        const dim3 sb((unsigned)((c->src.ns_pad + 255) / 256));
        dispatch<oa::FTILE_GROUPS, 64>(c->tile_groups, [&](auto TG) {
            hipLaunchKernelGGL((oa::k_nn_seed_sorted<decltype(TG)::value>), sb, dim3(256), 0, c->stream, (const oa::DevState *)c->d_state, (const float4 *)c->src.d_src4, c->src.ns_pad,
                               (const float4 *)c->tgt.d_tgs, (const float4 *)c->tgt.d_tfs, (const int4 *)c->tgt.d_tidx, c->tgt.n_groups_pad, c->sax[0], c->src.d_keys);
        });
        HIPCHK(hipGetLastError());
    }
    // every point's record at this pose, the waves' slots in the order of u (k_sorted_point_setup: once per search what every item of
    // the search used to work out for itself)
    {
        const dim3 ob((unsigned)(c->src.ns_pad / (64 * c->src.R)));
        dispatch<4, 1, 2, 8>(c->src.R, [&](auto R) {
            hipLaunchKernelGGL((oa::k_sorted_point_setup<decltype(R)::value>), ob, dim3(64), 0, c->stream, (const oa::DevState *)c->d_state, (const float4 *)c->src.d_src4,
                               (const float4 *)c->src.d_win, (const unsigned long long *)c->src.d_keys, c->sax[0], c->sax[1], pass, c->tune.nn_wave_order ? 1 : 0, c->src.ns_pad, c->src.ns, c->src.d_prec,
                               c->tgt.oct_c);                       // (the cap of the images this very search reads: oa_octgap.hpp)
        });
        HIPCHK(hipGetLastError());
    }
    // the blocks' home splits (the queue's order of items) and home tiles (where an item starts its visit of the split's tiles)
    {
        hipLaunchKernelGGL(oa::k_sorted_block_homes, dim3((unsigned)((std::max(q_blocks, oa::SORTED_QUEUES) + 63) / 64)), dim3(64), 0, c->stream,
                           (const oa::DevState *)c->d_state, (const float4 *)c->src.d_src4, q_blocks, oa::NN_THREADS * c->src.R, (const float4 *)c->tgt.d_tfs,
                           c->tgt.n_groups_pad, c->tile_groups, c->sax[0], q_splits, c->src.d_homes, c->src.d_qcnt);
        HIPCHK(hipGetLastError());
    }
    if (queued) sgrid = dim3((unsigned)q_wgs);
    auto launch = [&](auto R, auto TG, auto VCHUNK) {
        // level 0's own images: of 16 positions for the instances that fold them, else the pairs' (the per-vertex kind reads neither)
        const bool images = oa::sorted_level0(decltype(R)::value, decltype(VCHUNK)::value) == oa::Level0::Images;
        const float4 *l0 = images ? (const float4 *)c->tgt.d_toct : (const float4 *)c->tgt.d_tmw;
        hipLaunchKernelGGL((oa::k_nn_search_sorted<decltype(R)::value, decltype(TG)::value, decltype(VCHUNK)::value>), sgrid, dim3(oa::NN_THREADS), 0, c->stream,
                           c->d_state, (const float4 *)c->tgt.d_tgs, (const float4 *)c->tgt.d_tfs, (const float4 *)c->tgt.d_tf3s, (const int4 *)c->tgt.d_tidx,
                           c->tgt.n_groups_pad, c->src.d_keys, pass, (const float4 *)c->src.d_prec, q_splits, q_blocks, c->src.d_homes, queued ? c->src.d_qcnt : nullptr, c->tgt.nt, l0);
    };
    auto search = [&](auto R) { dispatch<oa::FTILE_GROUPS, 64>(c->tile_groups, [&](auto TG) { if (c->tune.nn_vchunk) launch(R, TG, yes); else launch(R, TG, no); }); };
#if defined(OA_EXPERIMENTS)
    dispatch<4, 1, 2, 8>(c->src.R, search);
#else
    dispatch<4, 1, 2>(c->src.R, search);                                // (8 points per thread: an OA_EXPERIMENTS instantiation; oa_create turns OA_NN_R=8 into 4)
#endif
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// brute force over the target's vertices: one thread per R source points, n_splits slices of the target
int launch_brute(oa_ctx *c, const SearchChoice &s)
{
    const dim3 grid(c->n_splits, c->src.ns_pad / (oa::NN_THREADS * c->src.R)), block(oa::NN_THREADS);
    if (grid.y > 65535)                                             // only the brute-force launch has this limit (grid.y)
        return fail(OA_E_BAD_ARG, "shard of %d points exceeds the brute-force launch grid (use more shards)", c->src.ns);
    switch (s.brute) {
    case BRUTE_SORTED: return launch_brute_sorted(c, grid);
#if defined(OA_EXPERIMENTS)
    case BRUTE_MFMA:
        dispatch<4, 2, 3>(c->tune.mfma_wps, [&](auto WPS) {
            hipLaunchKernelGGL((oa::k_nn_search_mfma<decltype(WPS)::value>), grid, block, 0, c->stream, c->d_state, c->src.d_src4, c->tgt.d_tg, (const oa::half8 *)c->tgt.d_tfm, (const float4 *)c->src.d_win, c->tgt.n_groups_pad, c->mfma_sigma, c->src.d_keys);
        });
        break;
    case BRUTE_FILTERED:
        dispatch<4, 1, 2, 8>(c->src.R, [&](auto R) {
            dispatch<oa::FTILE_GROUPS, 64>(c->tile_groups, [&](auto TG) {
                hipLaunchKernelGGL((oa::k_nn_search_filtered<decltype(R)::value, decltype(TG)::value>), grid, block, 0, c->stream, c->d_state, c->src.d_src4, c->tgt.d_tg, c->tgt.d_tf, c->tgt.d_tf3, (const float4 *)c->src.d_win, c->tgt.n_groups_pad, c->src.d_keys);
            });
        });
        break;
#endif
    default:
        dispatch<4, 1, 2, 8>(c->src.R, [&](auto R) {
            hipLaunchKernelGGL((oa::k_nn_search<decltype(R)::value>), grid, block, 0, c->stream, c->d_state, c->src.d_src4, c->tgt.d_tg, c->tgt.n_groups_pad, c->src.d_keys);
        });
        break;
    }
    HIPCHK(hipGetLastError());
    return OA_OK;
}

int launch_tri_search(oa_ctx *c, const SearchChoice &s, bool acc);
// One search of the shard as `s` says.  acc: the search also accumulates (launch_search_accumulate decided so: no accumulation
// launch follows)
int launch_nn(oa_ctx *c, const SearchChoice &s, bool acc)
{
    int rc = OA_OK;                                                 // (no points: nothing to search; the flags below are set all the same)
    if (c->src.ns > 0 && s.kind == SEARCH_TREE) rc = c->tgt.surface ? launch_bvh<true>(c, nullptr, nullptr, -1, acc) : launch_bvh<false>(c, nullptr, nullptr, -1, acc);
    else if (c->src.ns > 0 && c->tgt.surface) rc = launch_tri_search(c, s, acc);
    else if (c->src.ns > 0) rc = s.kind == SEARCH_GRID ? launch_vertex_grid(c, s, acc) : launch_brute(c, s);
    if (rc == OA_OK) { c->seeded = true; if (acc && !c->tgt.surface) c->win_seeds = true; }
    return rc;
}

// the plane metric's accumulation, and the weighted one of the point metric: one thread per source slot, workgroups by the
// shard size alone (every search mode leaves the same rows); begin_loop refuses shards beyond PLANE_MAX_BLOCKS rows
inline int plane_threads(const oa_ctx *c) { return c->src.ns >= 262144 ? oa::PLANE_THREADS : 256; }
inline int plane_blocks(const oa_ctx *c) { const int t = plane_threads(c); return std::max(1, (c->src.ns + t - 1) / t); }

// RECIP: every arm's variant that reads the verdict bytes (oa_set_reciprocal or oa_set_trim on); <false> launches what it always has
template <bool RECIP>
int launch_accumulate_as(oa_ctx *c, bool emit, int *nn_idx, float *nn_d2)
{
    if (!c->tgt.surface) c->win_seeds = true;                          // (the winner records of this pass seed the next search)
    oa::PairOut po{};
    const oa::PairTest<RECIP> nrm = pair_test<RECIP>(c);
    // the leading arguments of every kernel that opens with pair_fetch (oa_kernels.hpp); each arm adds its own behind them
    float4 *win = c->tgt.surface ? (float4 *)nullptr : c->src.d_win;
    const float4 *tri9 = c->tgt.surface ? (const float4 *)c->tgt.d_tri9 : (const float4 *)nullptr;
    const float *plane_tn = c->tgt.surface ? (const float *)nullptr : (const float *)c->tgt.d_tgt_n;
    // path: OA_ACC_* of the arm, for OA_STAT_ACC_PATH / _ROWS (one row of partials per workgroup)
    auto launch = [&](int path, auto *kern, int blocks, int threads, const auto &... tail) {
        c->last_acc_path = path; c->last_acc_rows = blocks;
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3((unsigned)threads), 0, c->stream, (const oa::DevState *)c->d_state,
                           (const float4 *)c->src.d_src4, c->src.ns, (const float *)c->tgt.d_tgt_xyz, c->src.d_keys, c->src.d_prev, win, tri9, nrm, tail...);
    };
    // the end of the search, for the step record (with the scale taken from the residuals, launch_robust_scale has stamped it)
    unsigned long long *stamp = c->loop_active ? &c->d_state->t_acc_start : (unsigned long long *)nullptr;
    unsigned long long *stamp_w = auto_scale(c) ? (unsigned long long *)nullptr : stamp;
    const float *w_slot = c->src.d_w;
    if (emit) {
        po.valid = c->src.d_valid; po.b = c->src.d_b; po.dist = c->src.d_dist; po.nn_idx = nn_idx; po.nn_d2 = nn_d2; po.perm = c->src.d_perm;
        launch(OA_ACC_STRIDE, oa::k_pair_accumulate<true, RECIP>, c->acc_blocks, oa::ACC_THREADS, c->d_partials, po, (unsigned long long *)nullptr);
    } else if (c->metric == OA_METRIC_PLANE) {
        auto *kern = weighted(c) ? oa::k_pair_accumulate_plane<true, RECIP> : oa::k_pair_accumulate_plane<false, RECIP>;
        launch(OA_ACC_PLANE, kern, plane_blocks(c), plane_threads(c), plane_tn, w_slot, c->d_partials, stamp_w);
    } else if (c->metric == OA_METRIC_GICP) {
        // (begin_loop refuses an estimated scale under this metric: the search always ends here)
        auto *kern = weighted(c) ? oa::k_pair_accumulate_gicp<true, RECIP> : oa::k_pair_accumulate_gicp<false, RECIP>;
        launch(OA_ACC_GICP, kern, plane_blocks(c), plane_threads(c), plane_tn, (const float *)c->src.d_src_n, w_slot, c->d_partials, stamp);
    } else if (c->metric == OA_METRIC_SYMMETRIC) {
        // (the plane kernel's row and epilogue: OA_ACC_PLANE)
        auto *kern = weighted(c) ? oa::k_pair_accumulate_symm<true, RECIP> : oa::k_pair_accumulate_symm<false, RECIP>;
        launch(OA_ACC_PLANE, kern, plane_blocks(c), plane_threads(c), plane_tn, (const float *)c->src.d_src_n, w_slot, c->d_partials, stamp_w);
    } else if (weighted(c)) {
        static_assert(oa::WEIGHTED_THREADS == oa::PLANE_THREADS, "plane_threads / plane_blocks size both launches");
        launch(OA_ACC_WEIGHTED, oa::k_pair_accumulate_weighted<RECIP>, plane_blocks(c), plane_threads(c), w_slot, c->d_partials, stamp_w);
    } else if (canon_blocks(c) > 0) {
        launch(OA_ACC_CANON, oa::k_pair_accumulate_canon<RECIP>, canon_blocks(c), canon_threads(c), canon_lanes(c), c->d_partials, stamp);
    } else {
        launch(OA_ACC_STRIDE, oa::k_pair_accumulate<false, RECIP>, c->acc_blocks, oa::ACC_THREADS, c->d_partials, po, stamp);
    }
    HIPCHK(hipGetLastError());
    return OA_OK;
}
int launch_accumulate(oa_ctx *c, bool emit, int *nn_idx, float *nn_d2)
{
    return verdict_on(c) ? launch_accumulate_as<true>(c, emit, nn_idx, nn_d2) : launch_accumulate_as<false>(c, emit, nn_idx, nn_d2);
}

// oa_set_robust_auto: between the search and the weighted accumulation of a loop step, the loss's scale from the residuals of
// the pairs that accumulation is about to form -- six launches, all on the loop's stream (oa_kernels.hpp, k_residual_keys)
// metric: whose residual (OA_METRIC_*; GICP: the trim's alone; symmetric: either's); hist: the level-0 counts of the select that follows
template <bool RECIP>
void launch_residual_keys(oa_ctx *c, int metric, uint32_t *hist)
{
    const oa::PairTest<RECIP> nrm = pair_test<RECIP>(c);
    // (launch_accumulate's selections; <false> never reads plane_tn)
    auto launch = [&](auto *kern, auto... tail) {
        launch_pair_reader(c, kern, (unsigned)plane_blocks(c), (unsigned)plane_threads(c), nrm, plane_tn(c), tail..., (const float *)c->src.d_w,
                           (uint32_t *)c->src.d_rkeys, hist, &c->d_state->t_acc_start);
    };
    if constexpr (RECIP) { if (metric == OA_METRIC_GICP) { launch(oa::k_residual_keys_gicp<true>, (const float *)c->src.d_src_n); return; } }
    if (metric == OA_METRIC_SYMMETRIC) { launch(oa::k_residual_keys_symm<RECIP>, (const float *)c->src.d_src_n); return; }
    if (metric == OA_METRIC_PLANE) launch(oa::k_residual_keys<true, RECIP>); else launch(oa::k_residual_keys<false, RECIP>);
}
// workgroups of a select's histogram launch: k_select_hist and k_dev_select_hist stride over the keys
inline unsigned select_hist_blocks(int ns) { return (unsigned)std::min(oa::SEL_HIST_MAX_BLOCKS, std::max(1, (ns + oa::SEL_THREADS - 1) / oa::SEL_THREADS)); }
// n_sel radix selects over keys[0 .. ns), one DevSelect and one block of SEL_LEVELS x SEL_BINS zeroed counts each (oa_deviation.hpp):
// per level the histogram, then the scan, on the context's stream.  level0_counted: the kernel that wrote the keys counted level 0
void launch_dev_select(oa_ctx *c, oa::DevSelect *sel, int n_sel, const uint32_t *keys, uint32_t *hist, bool level0_counted)
{
    for (int level = 0; level < oa::SEL_LEVELS; ++level) {
        if (level > 0 || !level0_counted)
            hipLaunchKernelGGL(oa::k_dev_select_hist, dim3(select_hist_blocks(c->src.ns), (unsigned)n_sel), dim3(oa::SEL_THREADS), 0, c->stream,
                               (const oa::DevSelect *)sel, keys, c->src.ns, level, hist);
        hipLaunchKernelGGL(oa::k_dev_select_scan, dim3((unsigned)n_sel), dim3(oa::SEL_THREADS), 0, c->stream, sel, (const uint32_t *)hist, level);
    }
}
int launch_robust_scale(oa_ctx *c)
{
    if (verdict_on(c)) launch_residual_keys<true>(c, c->metric, c->d_sel_hist); else launch_residual_keys<false>(c, c->metric, c->d_sel_hist);
    const unsigned hist_blocks = select_hist_blocks(c->src.ns);
    for (int level = 0; level < oa::SEL_LEVELS; ++level) {
        if (level > 0)
            hipLaunchKernelGGL(oa::k_select_hist, dim3(hist_blocks), dim3(oa::SEL_THREADS), 0, c->stream, (const oa::DevState *)c->d_state,
                               (const uint32_t *)c->src.d_rkeys, c->src.ns, level, c->d_sel_hist);
        hipLaunchKernelGGL(oa::k_select_scan, dim3(1), dim3(oa::SEL_THREADS), 0, c->stream, c->d_state, c->d_sel_hist, level);
    }
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// the trim's stage: the keys of the candidates, the cut (fixed share: the radix select with DevTrim::sel as its state; estimated:
// sort, prefix sums of r^2, argmin of J), the verdict bytes -- all on the loop's stream (oa_trim.hpp).  metric: whose residual
int launch_trim(oa_ctx *c, int metric)
{
    HIPCHK(hipMemsetAsync(c->d_trim_hist, 0, sizeof(uint32_t) * oa::SEL_LEVELS * oa::SEL_BINS, c->stream));
    launch_residual_keys<true>(c, metric, c->d_trim_hist);
    const oa::DevState *st = c->d_state;
    if (!trim_auto(c)) {
        launch_dev_select(c, &c->d_trim->sel, 1, (const uint32_t *)c->src.d_rkeys, c->d_trim_hist, true);
    } else {
        const int n_tiles = oa::trim_tiles(c->src.ns);
        // (all 32 bits: RKEY_NONE sorts last, and the one-workgroup sort and the LSD passes agree on every key)
        HIPCHK(oa::sort_order((void *)c->src.d_trim_tmp, (const uint32_t *)c->src.d_rkeys, c->src.d_trim_order, (size_t)c->src.ns, 32, c->stream));
        hipLaunchKernelGGL(oa::k_gather_int, dim3((unsigned)((c->src.ns + 255) / 256)), dim3(256), 0, c->stream, (const int *)c->src.d_rkeys,
                           (const int *)c->src.d_trim_order, c->src.ns, (int *)c->src.d_trim_sorted);
        hipLaunchKernelGGL(oa::k_trim_tile_sums, dim3((unsigned)n_tiles), dim3(oa::TRIM_THREADS), 0, c->stream, st, (const uint32_t *)c->src.d_trim_sorted, c->src.ns, c->src.d_trim_tiles);
        hipLaunchKernelGGL(oa::k_trim_tile_bases, dim3(1), dim3(oa::TRIM_BASE_THREADS), 0, c->stream, st, c->d_trim, (const uint32_t *)c->src.d_trim_sorted, c->src.ns,
                           c->src.d_trim_tiles, n_tiles);
        hipLaunchKernelGGL(oa::k_trim_apply, dim3((unsigned)n_tiles), dim3(oa::TRIM_THREADS), 0, c->stream, st, (const oa::DevTrim *)c->d_trim,
                           (const uint32_t *)c->src.d_trim_sorted, c->src.ns, (const double *)c->src.d_trim_tiles, c->src.d_trim_min);
        hipLaunchKernelGGL(oa::k_trim_argmin, dim3(1), dim3(oa::TRIM_THREADS), 0, c->stream, st, c->d_trim, (const uint32_t *)c->src.d_trim_sorted,
                           (const oa::TrimTileMin *)c->src.d_trim_min, n_tiles);
    }
    const unsigned vblocks = (unsigned)std::min(oa::TRIM_VERDICT_MAX_BLOCKS, std::max(1, (c->src.ns + oa::TRIM_THREADS - 1) / oa::TRIM_THREADS));
    hipLaunchKernelGGL(oa::k_trim_verdict, dim3(vblocks), dim3(oa::TRIM_THREADS), 0, c->stream, st, c->d_trim, (const uint32_t *)c->src.d_rkeys, c->src.ns, c->src.d_recip_ok);
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// The filters' stages of one step, on the step's stream: search -> k_recip_check -> k_boundary_verdict -> the trim ->
// [launch_robust_scale, over the survivors] -> the accumulation.  This function alone holds the order and decides who
// writes the verdict bytes first: k_recip_check writes every byte; without it the bytes are set to 1 ahead of the first stage that
// is on, and every later stage only takes pairs away.  metric, metric_n: the accumulation that follows (whose residual the trim
// cuts on, and its pair_fetch<.., METRIC_N>); oa_make_pairs does not look at the metric: the point residual
int launch_filters(oa_ctx *c, int metric, bool metric_n)
{
    int rc;
    if (!verdict_on(c) || c->src.ns <= 0) return OA_OK;                 // (no slot to judge: nothing is allocated for it either, ensure_filters)
    if (!c->recip_on) HIPCHK(hipMemsetAsync(c->src.d_recip_ok, 1, (size_t)c->src.ns, c->stream));
    if (c->recip_on && (rc = launch_recip(c, metric_n))) return rc;
    if (c->bnd_on && (rc = launch_boundary(c))) return rc;
    if (trim_on(c) && (rc = launch_trim(c, metric))) return rc;
    return OA_OK;
}

// rows the (non-emitting) accumulation of this context leaves for the reduce launch when it is its own kernel
inline oa::RowSel plain_rows(const oa_ctx *c)
{
    if (plane_row_metric(c) || weighted(c)) return oa::RowSel{ plane_blocks(c), 0, 0 };
    const int cb = canon_blocks(c);
    return oa::RowSel{ cb > 0 ? cb : c->acc_blocks, 0, 0 };
}

// rows of partials -> d_sums.  stamp: the launch marks the end of the search + accumulate part (fused searches)
int launch_reduce(oa_ctx *c, double *d_sums, const oa::RowSel &sel, bool stamp)
{
    hipLaunchKernelGGL(oa::k_reduce_partials, dim3(1), dim3(oa::RED_THREADS), 0, c->stream, (const oa::DevState *)c->d_state,
                       (const double *)c->d_partials, sel, d_sums, stamp ? &c->d_state->t_acc_start : (unsigned long long *)nullptr);
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// search + accumulate of one iteration, by the plan above; sel = the rows the reduce launch finds; fused = no separate
// accumulation launch ran (the reduce launch then stamps the end of the search part)
int launch_search_accumulate(oa_ctx *c, bool timed, oa::RowSel &sel, bool &fused)
{
    int rc;
    // hipEvent pairs around the search cost ~7 us of stream time per iteration (two barrier packets): fine for the
    // brute-force kernel (50 ms per launch), not for the grid / tree searches, whose launches are that short
    // themselves -- those are timed on the GPU instead (DevState::t_prev_end / t_acc_start, StepRecord::search_ticks)
    timed = timed && c->time_events;
    const SearchChoice s = choose_search(c);
    fused = s.plan == PLAN_TREE || s.plan == PLAN_DUAL || (s.plan == PLAN_GRID && grid_fast_now(c));
    c->iter_enq++;
    // the lazy safe radii: counted once per iteration, whatever the plan launches (tree and grid in turns count once; shards too
    // large for the fused path -- BASELINE config 5 on one GPU -- count too: their plain grid search takes seeds on their radii
    // all the same); brute force never reads them
    if (!c->tgt.surface && c->tgt.grid_ok && c->grid_mode != 0) { ++c->tgt.target_iters; if ((rc = safe_radii_lazy(c))) return rc; }
    if (s.plan == PLAN_GRID && fused) c->fast_iters++;
    if (timed) {
        if ((rc = ensure_events(c, c->ev_used + 1))) return rc;
        HIPCHK(hipEventRecord(c->ev[2 * c->ev_used], c->stream));
    }
    if ((rc = launch_nn(c, s, fused))) return rc;
    if (timed) {
        HIPCHK(hipEventRecord(c->ev[2 * c->ev_used + 1], c->stream));
        c->ev_used++;
    }
    if (!fused) {
        if ((rc = launch_filters(c, c->metric, plane_row_metric(c)))) return rc;
        if (auto_scale(c) && (rc = launch_robust_scale(c))) return rc;
        if ((rc = launch_accumulate(c, false, nullptr, nullptr))) return rc;
        sel = plain_rows(c);
        return OA_OK;
    }
    const int tree_rows = (int)bvh_blocks(c, false, true);
    if (s.plan == PLAN_TREE) sel = oa::RowSel{ tree_rows, 0, 0 };
    else sel = oa::RowSel{ canon_blocks(c), s.plan == PLAN_DUAL ? tree_rows : 0, s.plan == PLAN_DUAL ? 1 : 0 };
    c->last_acc_path = s.plan == PLAN_TREE ? (c->tgt.surface ? OA_ACC_FUSED_TRI_TREE : OA_ACC_FUSED_TREE)
                       : s.plan == PLAN_DUAL ? OA_ACC_DUAL : (c->tgt.surface ? OA_ACC_FUSED_TRI_GRID : OA_ACC_FUSED_GRID);
    c->last_acc_rows = sel.n;
    return OA_OK;
}

// smallest singular value of the upper-left 3x3 of a row-major 4x4 (cyclic Jacobi on M^T M, double)
double min_singular_3x3(const float *M)
{
    double S[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double a = 0.0;
            for (int k = 0; k < 3; ++k) a += (double)M[4 * k + i] * (double)M[4 * k + j];
            S[i][j] = a;
        }
    for (int sweep = 0; sweep < 30; ++sweep) {
        const double off = fabs(S[0][1]) + fabs(S[0][2]) + fabs(S[1][2]);
        if (!(off > 1e-300)) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (S[p][q] == 0.0) continue;
                const double theta = (S[q][q] - S[p][p]) / (2.0 * S[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < 3; ++k) { const double a = S[k][p], b = S[k][q]; S[k][p] = cs * a - sn * b; S[k][q] = sn * a + cs * b; }
                for (int k = 0; k < 3; ++k) { const double a = S[p][k], b = S[q][k]; S[p][k] = cs * a - sn * b; S[q][k] = sn * a + cs * b; }
            }
    }
    double m = std::min(S[0][0], std::min(S[1][1], S[2][2]));
    if (!(m > 0.0)) return 0.0;
    return sqrt(m);
}

// The search radius of the grid / tree searches for a given thresh (DevState::cut_a / cut_b, search_cutoff2) and
// 1 / sigma_min(mx2); the arguments are left as they are where no radius applies.
void search_radius(const oa_ctx *c, const float *mx2, double thresh, double &cut_a, double &cut_b, double &local_per_world)
{
    if (!(c->tgt.filter_ok && c->grid_mode != 0 && c->tune.nn_cutoff)) return;
    const double smin = min_singular_3x3(mx2) * (1.0 - 1e-9);
    if (smin > 0.0) local_per_world = 1.0 / smin;
    double m2norm = 0.0, tmax = 0.0, tscale = 0.0;
    for (int i = 0; i < 3; ++i) {
        m2norm = std::max(m2norm, fabs((double)mx2[4 * i]) + fabs((double)mx2[4 * i + 1]) + fabs((double)mx2[4 * i + 2]));
        tmax = std::max(tmax, fabs((double)mx2[4 * i + 3]));
        tscale = std::max(tscale, std::max(fabs(c->bb_lo[i]), fabs(c->bb_hi[i])));
    }
    const double u64 = 64.0 * 5.9604644775390625e-08;
    if (smin > 0.0 && thresh > 0.0 && thresh < 1e300) {
        cut_a = (thresh + u64 * (m2norm * 3.0 * tscale + tmax)) / smin * (1.0 + 1e-5);
        cut_b = u64 * m2norm / smin * (1.0 + 1e-5);
        if (!(cut_a < 1e300) || !(cut_b < 1e300)) { cut_a = INFINITY; cut_b = 0.0; }
    }
}

const float EYE16[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };   // the 4 x 4 identity

// DevState / PoseBatch::mx2_identity: the target's matrix is the identity, bit for bit -- the searches skip its products
int mx2_identity(const oa_ctx *c, const float *mx2)
{
    return (memcmp(mx2, EYE16, sizeof EYE16) == 0 && !c->tune.no_identity_path) ? 1 : 0;
}

void init_loop_state(oa_ctx *c, const oa_settings *st, int iters, bool cutoff = true)
{
    oa::DevState &s = c->h_state;
    // search radius (DevState::cut_a / cut_b): only the grid / tree searches use it
    s.cut_a = INFINITY; s.cut_b = 0.0;
    s.local_per_world = 0.0;
    s.host_halt = nullptr;
    c->poll_mapped = false;
    s.t_prev_end = 0; s.t_acc_start = 0;
    s.t_xchg_start = 0;                                             // (a stale stamp would leak into the first exchange_ticks of this loop)
    s.search_clk[0] = 0; s.search_clk[1] = 0;                       // OA_STAT_SEARCH_CLOCK_MHZ: 0 unless THIS loop's search stamps it
    {   // first search of a loop: the tree (cold or stale seeds); a one-shot call on warm seeds: the grid
        const bool grid_up = c->tgt.surface ? c->tgt.tri_grid_ok : c->tgt.grid_ok;
        const oa::GridParams &g = c->tgt.surface ? c->tgt.tgp : c->tgt.gp;
        s.turn_limit = grid_up ? c->tune.turn_frac * g.h : 0.0;
        s.turn_scale = grid_up ? g.scale : 0.0;
        s.tree_turn = (iters > 1 || !c->seeded) ? 1 : 0;
        s.mx2_identity = mx2_identity(c, s.mx2);
    }
    if (c->h_poll) {
        void *dp = nullptr;
        if (hipHostGetDevicePointer(&dp, c->h_poll, 0) == hipSuccess) { s.host_halt = (int32_t *)dp; c->poll_mapped = true; }
        else (void)hipGetLastError();
    }
    if (cutoff) search_radius(c, s.mx2, st->thresh, s.cut_a, s.cut_b, s.local_per_world);
    for (int k = 0; k < 3; ++k) s.pivot[k] = c->src.pivot[k];
    s.thresh = st->thresh;
    s.target_d = st->target_d;
    for (int k = 0; k < 5; ++k) { s.ring_t[k] = st->target_d * 2.0; s.ring_r[k] = 0.0; }   // icp_align.py:93-94
    s.iters = iters;
    s.use_target = st->use_target ? 1 : 0;
    s.with_scale = st->with_scale ? 1 : 0;
    s.early_exit = st->early_exit ? 1 : 0;
    s.n = 0; s.converged = 0; s.status = 0; s.halt = (iters <= 0) ? 1 : 0;
    s.max_records = c->max_records; s.pad0 = 0;
    for (int k = 0; k < 3; ++k) { s.tc[k] = c->tc[k]; s.fax[k] = c->fax[k]; }
    s.pad1 = 0.f; s.pad2 = 0;
    s.qmax = c->qmax;
    s.d_pivot = c->d_pivot0;
    s.jac_valid = 0; s.plane_rank = 0;                                    // every loop starts its Jacobi from the identity
    for (int k = 0; k < 9; ++k) s.jac_v[k] = 0.0;
    s.weighted = weighted(c) ? 1 : 0;
    s.loss = c->loss;
    s.robust_c = c->robust_c;
    {   // the plane residual is in align-local units, the loss's scale in world units: cbrt(|det|) of the float32 matrix, in fp64
        // (the plane step is rigid: the determinant does not change during a loop)
        const float *m = s.mx1;
        const double det = (double)m[0] * ((double)m[5] * (double)m[10] - (double)m[6] * (double)m[9])
                         - (double)m[1] * ((double)m[4] * (double)m[10] - (double)m[6] * (double)m[8])
                         + (double)m[2] * ((double)m[4] * (double)m[9] - (double)m[5] * (double)m[8]);
        s.res_scale = cbrt(fabs(det));
    }
    s.weight_sum = 0.0;
    s.gicp_eps = c->gicp_eps;
    s.symmetric = c->metric == OA_METRIC_SYMMETRIC ? 1 : 0;
    s.pad4 = 0;
    // the scale from the residuals: robust_c is then the multiplier, and k_select_scan writes the scale before every accumulation
    const bool auto_c = auto_scale(c);
    s.robust_mult = auto_c ? c->robust_c : 0.0;
    s.robust_p = auto_c ? c->robust_p : 0.0;
    s.robust_cmin = auto_c ? c->robust_cmin : 0.0;
    if (auto_c) s.robust_c = c->robust_cmin;
    s.robust_q = 0.0;
    s.robust_kq = 0; s.sel_prefix = 0; s.sel_rank = 0; s.pad3 = 0;
}

// oa_iterate opens a loop without an end; its history is a ring of the last ITERATE_RING iterations
constexpr int ITERATE_OPEN = 0x7FFFFFFF, ITERATE_RING = 64;

int begin_loop(oa_ctx *c, const oa_settings *st, int iters)
{
    int rc = check_ready(c);
    if (rc) return rc;
    if (!st) return fail(OA_E_BAD_ARG, "null settings");
    if (!(st->thresh > 0.0)) return fail(OA_E_BAD_THRESH, "thresh must be > 0 (the reference's make_pairs returns None)");
    if (const char *noun = normal_metric_noun(c->metric)) {            // the metrics that read normals: a rigid step, and the wider row
        if (st->with_scale) return fail(OA_E_BAD_ARG, "the %s metric solves for a rigid step: with_scale must be 0 (or call oa_set_metric(ctx, OA_METRIC_POINT))", noun);
        if (!c->tgt.surface && !c->tgt.d_tgt_n)
            return fail(OA_E_STATE, "the %s metric needs target normals: call oa_set_target_normals (or oa_set_normals) after oa_set_target, or upload a mesh with oa_set_target_mesh", noun);
        if (c->metric != OA_METRIC_PLANE && !c->src.d_src_n)          // (the plane metric reads the target's alone)
            return fail(OA_E_STATE, "the %s metric needs source normals: call oa_set_source_normals (or oa_set_normals) after oa_set_source", noun);
        if (c->metric == OA_METRIC_GICP && auto_scale(c))             // (GICP alone: its loss takes a fixed scale)
            return fail(OA_E_STATE, "the GICP metric takes a robust loss with a fixed scale only: call oa_set_robust_auto(ctx, 0, 0) (or oa_set_metric(ctx, OA_METRIC_PLANE))");
        if ((long long)c->src.ns > (long long)oa::PLANE_MAX_BLOCKS * oa::PLANE_THREADS)
            return fail(OA_E_CAPACITY, "the %s metric takes shards of up to %lld points (this one: %d): use more shards", noun, (long long)oa::PLANE_MAX_BLOCKS * oa::PLANE_THREADS, c->src.ns);
    } else if (weighted(c) && (long long)c->src.ns > (long long)oa::PLANE_MAX_BLOCKS * oa::WEIGHTED_THREADS)
        return fail(OA_E_CAPACITY, "a weighted loop takes shards of up to %lld points (this one: %d): use more shards", (long long)oa::PLANE_MAX_BLOCKS * oa::WEIGHTED_THREADS, c->src.ns);
    if ((rc = refuse_filters_shard(c, "a loop"))) return rc;
    if ((rc = use_device(c))) return rc;
    if ((rc = ensure_common(c))) return rc;
    if ((rc = ensure_filters(c))) return rc;
    if ((rc = ensure_history(c, iters == ITERATE_OPEN ? ITERATE_RING : iters))) return rc;   // oa_iterate: a small ring
    if (auto_scale(c)) {                                          // the selection's buffers; its histograms start (and are kept) at zero
        if (!c->src.d_rkeys) HIPCHK(dev_malloc(&c->src.d_rkeys, sizeof(uint32_t) * (size_t)std::max(1, c->src.ns)));
        if (!c->d_sel_hist) HIPCHK(dev_malloc(&c->d_sel_hist, sizeof(uint32_t) * oa::SEL_LEVELS * oa::SEL_BINS));
        HIPCHK(hipMemsetAsync(c->d_sel_hist, 0, sizeof(uint32_t) * oa::SEL_LEVELS * oa::SEL_BINS, c->stream));
    }
    c->settings = *st;
    c->iterate_mode = false;
    HIPCHK(hipStreamSynchronize(c->stream));                    // nothing of an earlier loop may still write the host flag
    if (c->h_poll) { for (int k = 0; k < 8; ++k) c->h_poll[k] = 0; }
    init_loop_state(c, st, iters);
    *c->h_state_pin = c->h_state;                               // pinned staging copy (the stream is idle, see above)
    HIPCHK(hipMemcpyAsync(c->d_state, c->h_state_pin, sizeof(oa::DevState), hipMemcpyHostToDevice, c->stream));
    if (c->src.d_todo_count) HIPCHK(hipMemsetAsync(c->src.d_todo_count, 0, TODO_COUNT_INTS * sizeof(int), c->stream));   // kept at zero by k_solve_update (the front search's counters: by its launches)
    c->src.u_slot = 0;
    if (!c->tgt.surface && (rc = safe_radii_lazy(c))) return rc;
    hipLaunchKernelGGL(oa::k_stamp_start, dim3(1), dim3(64), 0, c->stream, c->d_state);
    HIPCHK(hipGetLastError());
    c->ev_used = 0;
    c->iter_enq = 0;
    c->fast_iters = 0;
    c->h_hist_valid = false;
    {
        // (surfaces: NOT kind == SEARCH_BRUTE -- a mesh with a tree but no grid counts as a tree search here, as it always has)
        const bool brute = !c->tgt.surface ? choose_search(c).kind == SEARCH_BRUTE : (c->grid_mode == 0 || !c->tgt.tbvh_ok);
        c->time_events = c->tune.time_events < 0 ? brute : c->tune.time_events != 0;
    }
    c->loop_active = true;
    return OA_OK;
}

int iter_partial(oa_ctx *c, double *d_sums, bool timed)
{
    oa::RowSel sel;
    bool fused;
    const int rc = launch_search_accumulate(c, timed, sel, fused);
    if (rc) return rc;
    return launch_reduce(c, d_sums, sel, fused);
}

int iter_finish(oa_ctx *c, const double *d_sums)
{
    hipLaunchKernelGGL(oa::k_solve_update, dim3(1), dim3(128), 0, c->stream, c->d_state, d_sums, c->d_hist, c->src.d_todo_count);
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// single-GPU iteration: search (+ accumulate), then reduce + solve in one launch
int iter_fused(oa_ctx *c, bool timed)
{
    oa::RowSel sel;
    bool fused;
    const int rc = launch_search_accumulate(c, timed, sel, fused);
    if (rc) return rc;
    if (plane_row_metric(c))
        hipLaunchKernelGGL(oa::k_reduce_solve_update_plane, dim3(1), dim3(oa::RED_THREADS), 0, c->stream, c->d_state,
                           (const double *)c->d_partials, sel.n, c->d_sums, c->d_hist, c->src.d_todo_count);
    else
        hipLaunchKernelGGL(oa::k_reduce_solve_update, dim3(1), dim3(oa::RED_THREADS), 0, c->stream, c->d_state,
                           (const double *)c->d_partials, sel, c->d_sums, c->d_hist, c->src.d_todo_count, fused ? 1 : 0);
    HIPCHK(hipGetLastError());
    return OA_OK;
}

int fetch_state(oa_ctx *c)
{
    HIPCHK(hipMemcpyAsync(c->h_state_pin, c->d_state, sizeof(oa::DevState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->h_state = *c->h_state_pin;
    if (plane_row_metric(c) && c->h_state.n > 0) c->last_plane_rank = c->h_state.plane_rank;
    if (c->h_state.n > 0) c->last_weight_sum = c->h_state.weight_sum;
    if (c->h_state.n > 0) c->last_robust_c = c->h_state.robust_c;
    return OA_OK;
}

// host mirror -> device through the pinned staging copy (the stream must be idle: the staging copy is reused)
int push_state(oa_ctx *c)
{
    *c->h_state_pin = c->h_state;
    HIPCHK(hipMemcpyAsync(c->d_state, c->h_state_pin, sizeof(oa::DevState), hipMemcpyHostToDevice, c->stream));
    return OA_OK;
}

int fill_report(oa_ctx *c, oa_report *rep)
{
    int rc = fetch_state(c);
    if (rc) return rc;
    const oa::DevState &s = c->h_state;
    memset(rep, 0, sizeof *rep);
    if (c->h_poll && s.n > 0) c->last_todo_wave_max = c->h_poll[3];   // where the next loop's first grid search starts from (grid_fast_now)
    rep->iters_done = s.n;
    rep->converged = s.converged;
    rep->status = s.status;
    rep->mean_dist = rep->std_dist = NAN;
    c->h_hist_valid = false;
    const int m = (s.n > 0 && c->d_hist) ? std::min(s.n, c->max_records) : 0;
    if (m > 0) {                                                  // one copy serves the report, the timing and oa_get_history
        c->h_hist.resize((size_t)m);
        memcpy(c->h_hist.data(), c->h_hist_map, sizeof(oa::StepRecord) * (size_t)m);   // the stream is idle: fetch_state synchronised
        c->h_hist_valid = true;
        const oa::StepRecord &r = c->h_hist[(size_t)((s.n - 1) % c->max_records)];
        rep->last_K = (int64_t)r.K;
        rep->last_translation = r.trans;
        if (s.use_target) { rep->mean_dist = r.mean_d; rep->std_dist = r.std_d; }
        double a = 0.0;
        const int mm = std::min(s.n, 5);
        if (s.use_target) { for (int k = 0; k < mm; ++k) a += s.ring_r[k]; rep->mean_rot_angle = a / mm; }
        else rep->mean_rot_angle = r.angle;
    }
    // search time: hipEvent pairs around every launch (brute force), else the GPU-side stamps the loop left in the
    // step records (end of the previous iteration -> start of k_pair_accumulate)
    double nn_ms = 0.0;
    c->h_search_ms.clear();                                       // per launch, for oa_get_search_ms
    if (c->time_events) {
        for (int k = 0; k < c->ev_used; ++k) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c->ev[2 * k], c->ev[2 * k + 1]) == hipSuccess) { nn_ms += ms; c->h_search_ms.push_back((double)ms); }
        }
    } else if (m > 0) {
        double ticks = 0.0;
        for (int k = 0; k < m; ++k) { ticks += c->h_hist[(size_t)k].search_ticks; c->h_search_ms.push_back(c->h_hist[(size_t)k].search_ticks / c->wall_clock_khz); }
        nn_ms = ticks / c->wall_clock_khz * ((double)s.n / (double)m);
    }
    rep->nn_ms_total = nn_ms;
    // multi-GPU: how long the device waited for the world's sums, per iteration (StepRecord::exchange_ticks)
    c->last_exchange_us = 0.0;
    if (m > 0) {
        double ticks = 0.0;
        for (int k = 0; k < m; ++k) ticks += c->h_hist[(size_t)k].exchange_ticks;
        c->last_exchange_us = ticks / c->wall_clock_khz * 1e3 / (double)m;
    }
    return OA_OK;
}


// ------------------------------------------------------------------------------------------------
// multi-device exchange: how the children of an oa_create_multi context join their sums
// ------------------------------------------------------------------------------------------------
//   OA_EXCHANGE_RCCL     ncclAllReduce(24 doubles, sum) over xGMI on every device's stream through a single-process
//                        ncclCommInitAll communicator (librccl is loaded on first use: liboa_icp.so does not link it).
//                        What BASELINE.json's north-star names; the DEFAULT whenever the listed devices are distinct and
//                        librccl can be brought up (OA_EXCHANGE_AUTO).
//   OA_EXCHANGE_MAILBOX  one-shot all-gather through mailboxes: k_reduce_post writes a rank's 24 sums + a sequence word
//                        into every rank's inbox, k_gather_solve_update waits for the world's posts in its own inbox and
//                        adds them in rank order (bitwise identical on every device).  No host involvement, no extra
//                        launches: an iteration stays search -> accumulate -> post -> solve.  The inboxes live in device
//                        memory (fine-grained, peer-mapped: the 200 B travel over xGMI and every rank polls its own HBM);
//                        when peer access is not available, one box in pinned host memory every device maps (PCIe).
//                        The fallback of AUTO: duplicate devices (one-GPU test boxes), no librccl.
}  // namespace
struct oa_exchange {
    int world = 0;
    int requested = OA_EXCHANGE_AUTO;              // what the caller asked for (env OA_EXCHANGE / oa_set_exchange)
    int mode = OA_EXCHANGE_MAILBOX;                // what the loops use once `resolved`
    bool resolved = false;
    std::string auto_note;                         // why AUTO did not take RCCL
    // mailbox
    bool device_box = false;                       // inboxes in device memory (peer-mapped) instead of the pinned host box
    oa::MailSlot *h_box = nullptr;                 // host box [2][world]
    std::vector<oa::MailSlot *> box;               // rank r's mailbox as rank r's device sees it (its inbox / the host box)
    std::vector<oa::MailSlot **> d_dests;          // rank r: device array of the mailboxes r posts into
    int n_dest = 1;
    unsigned long long timeout_ticks = 0;
    unsigned long long seq_next = 0;               // DevState::seq_base of the next loop
    int fault_skip_rank = -1;                      // OA_FAULT_SKIP_POST_RANK: that rank's posts never arrive (test hook)
    double timeout_s = 30.0;                       // OA_EXCHANGE_TIMEOUT_S: the mailbox kernels' wait (timeout_ticks) and the host's watchdog in RCCL mode
    // How many iterations the host threads of one oa_run enqueue: agreed, not observed.  Every thread stops on what ITS device
    // reports (DevState::host_halt), and the threads hear of a halt at different times; an iteration enqueued in RCCL mode
    // contains a collective, and a collective one rank enqueues and another does not never completes.  So: a thread COMMITS
    // to iteration `it` under the lock before it enqueues it (agree_committed = most iterations any thread has committed to);
    // the first thread that hears of the halt -- or fails -- freezes agree_stop_at = agree_committed; from then on every
    // thread enqueues exactly agree_stop_at iterations, no more (it stops there) and no fewer (it tops up to it: iterations
    // after the halt are empty but for the collective).  The count is a function of the lock order alone, never of what a
    // thread happened to read from its device afterwards.  (multi_group_loop; docs/HISTORY.md 4.7 "the invariant")
    std::mutex agree_mu;
    int agree_committed = 0;
    std::atomic<int> agree_stop_at{ -1 };          // -1: not frozen yet
    bool agree_on = true;                          // OA_MULTI_AGREE=0 (test hook, ignored in RCCL mode): round 3's every-thread-for-itself stop
    int fault_lag_group = -1, fault_lag_us = 0;    // OA_FAULT_LAG_GROUP / OA_FAULT_LAG_US: that host thread sleeps before every look at its halt flag (test hook)
    // (atomics: every host thread looks at these, the one they name clears them once they have fired -- a plain int was a
    //  data race, found by the ThreadSanitizer pass of round 4, profiles/r04d_sanitizers.txt)
    std::atomic<int> fault_fail_group{ -1 };           // OA_FAULT_FAIL_GROUP / OA_FAULT_FAIL_ITER: that host thread's enqueue fails at that iteration (test hook)
    int fault_fail_iter = -1;
    std::atomic<int> fault_stall_rank{ -1 };           // OA_FAULT_STALL_RANK / _ITER: that rank's stream stops ahead of its collective, as if its peers never arrived (test hook)
    int fault_stall_iter = 2;
    int32_t *h_release = nullptr;                  // pinned word the stalled stream watches: exchange_abort_rccl releases it
    // RCCL
    void *lib = nullptr;
    std::vector<ncclComm_t> comms;
    int rccl_ranks_last = 0;                       // ranks of the last communicator that came up and passed its handshake (it may have been aborted since)
    int rccl_fallbacks = 0;                        // loops that AUTO started on RCCL and finished through the mailboxes (multi_run)
    bool rccl_aborted = false;                     // a loop ran into the watchdog and the communicators were aborted: AUTO stays on the mailbox from here on
    long long watchdog_aborts = 0;                 // OA_STAT_WATCHDOG_ABORTS
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
    ncclResult_t (*CommGetAsyncError)(ncclComm_t, ncclResult_t *) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
namespace {
using Exchange = oa_exchange;

#define RCCLCHK(x, expr)                                                                                         \
    do {                                                                                                         \
        ncclResult_t r_ = (expr);                                                                                \
        if (r_ != ncclSuccess)                                                                                   \
            return fail(OA_E_RCCL, "%s failed: %s", #expr, (x)->GetErrorString ? (x)->GetErrorString(r_) : "?"); \
    } while (0)

bool devices_distinct(const oa_ctx *p)
{
    for (size_t i = 0; i < p->subs.size(); ++i)
        for (size_t j = 0; j < i; ++j)
            if (p->subs[i]->device == p->subs[j]->device) return false;
    return true;
}

// RCCL's communicators are given up: every collective kernel still waiting for a peer returns, the streams drain.
// (ncclCommAbort frees the communicator; the next explicit oa_set_exchange(RCCL) builds new ones.)
void exchange_abort_rccl(oa_ctx *p, const char *why)
{
    Exchange *x = p->xch;
    if (x->h_release) { __atomic_store_n(x->h_release, 1, __ATOMIC_RELEASE); }   // (test hook: the stalled stream goes on)
    if (x->comms.empty()) return;
    if (p->subs.empty() ? false : p->subs[0]->tune.debug) fprintf(stderr, "[oa] RCCL communicators aborted: %s\n", why);
    for (size_t i = 0; i < x->comms.size(); ++i)
        if (x->comms[i] && x->CommAbort) { if (i < p->subs.size()) (void)hipSetDevice(p->subs[i]->device); (void)x->CommAbort(x->comms[i]); }
    x->comms.clear();
    x->rccl_aborted = true;
    x->watchdog_aborts++;
    x->resolved = false;                             // AUTO resolves to the mailbox from here on (exchange_resolve)
    x->auto_note = std::string("RCCL was aborted: ") + why;
}

// Wait for every child's stream, never for ever.  Mailbox: the gather kernels bound their own wait (timeout_ticks), so a
// plain synchronise returns.  RCCL: a collective whose peers never enter it spins until its communicator is aborted, so
// the host watches the streams (hipStreamQuery) and the devices' progress words; when no device has finished an
// iteration for OA_EXCHANGE_TIMEOUT_S -- or RCCL reports an asynchronous error -- it aborts the communicators
// (ncclCommAbort), gives the streams the same time again to drain, and the call fails with OA_E_RCCL.
// abort_now: the caller knows the ranks' collective counts differ (a host thread failed mid-loop): no point in waiting.
int multi_wait(oa_ctx *p, bool abort_now = false, bool in_loop = true)
{
    Exchange *x = p->xch;
    const size_t n = p->subs.size();
    const bool rccl = x && x->mode == OA_EXCHANGE_RCCL && !x->comms.empty();
    if (!rccl) {
        int rc = OA_OK;
        for (oa_ctx *c : p->subs) {
            hipError_t e = hipSetDevice(c->device);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess && !rc) rc = fail(OA_E_HIP, "device %d: %s", c->device, hipGetErrorString(e));
        }
        return rc;
    }
    using clk = std::chrono::steady_clock;
    const auto limit = std::chrono::duration<double>(x->timeout_s);
    std::vector<char> done(n, 0);
    std::vector<int> seen(n, -1);
    bool aborted = false;
    std::string why;
    if (abort_now) { exchange_abort_rccl(p, "a host thread failed while the loop was being enqueued"); aborted = true; why = "a host thread failed mid-loop"; }
    auto t_last = clk::now();
    for (;;) {
        // The clock runs while SOME stream sits in its exchange (h_poll[5] > h_poll[1]: k_reduce_partials has run, the solve behind
        // the collective has not) and nothing moves; a device that is still searching -- a 10M-point brute-force shard takes
        // seconds per iteration -- is not a stalled collective.  in_loop = false: the handshake, which is nothing but a collective.
        bool all = true, moved = false, waiting = !in_loop || aborted;
        for (size_t i = 0; i < n; ++i) {
            if (done[i]) continue;
            oa_ctx *c = p->subs[i];
            hipError_t e = hipSetDevice(c->device);
            if (e == hipSuccess) e = hipStreamQuery(c->stream);
            if (e == hipSuccess) { done[i] = 1; moved = true; continue; }
            if (e != hipErrorNotReady) { (void)hipGetLastError(); return fail(OA_E_HIP, "device %d: %s", c->device, hipGetErrorString(e)); }
            (void)hipGetLastError();
            all = false;
            const int at = c->h_poll ? ((volatile int32_t *)c->h_poll)[1] : 0;
            if (at != seen[i]) { seen[i] = at; moved = true; }
            // (a child whose progress words are not mapped can never show "in its exchange": it counts as waiting, so that a
            //  hung collective is still aborted -- the clock then also runs through its searches, as before round 5)
            if (!c->h_poll || !c->poll_mapped || ((volatile int32_t *)c->h_poll)[5] > at) waiting = true;
            if (!aborted && x->CommGetAsyncError && i < x->comms.size() && x->comms[i]) {
                ncclResult_t ar = ncclSuccess;
                if (x->CommGetAsyncError(x->comms[i], &ar) == ncclSuccess && ar != ncclSuccess && ar != ncclInProgress) {
                    why = std::string("RCCL reported an asynchronous error on device ") + std::to_string(c->device) + ": " + (x->GetErrorString ? x->GetErrorString(ar) : "?");
                    exchange_abort_rccl(p, why.c_str());
                    aborted = true; t_last = clk::now();
                }
            }
        }
        if (all) break;
        if (moved || !waiting) t_last = clk::now();
        else if (clk::now() - t_last > limit) {
            if (aborted) return fail(OA_E_RCCL, "multi-device exchange: %s, and the streams did not drain within %.1f s of the abort", why.c_str(), x->timeout_s);
            why = "no device finished an iteration for " + std::to_string(x->timeout_s) + " s (OA_EXCHANGE_TIMEOUT_S)";
            exchange_abort_rccl(p, why.c_str());
            aborted = true; t_last = clk::now();
        }
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    if (aborted) return fail(OA_E_RCCL, "multi-device exchange: %s; the RCCL communicators were aborted", why.c_str());
    return OA_OK;
}

// first use of new communicators: one all-reduce of a known value on every device, waited for with the watchdog.  A
// communicator that cannot do that (a link down, a peer mapping refused) is aborted here -- AUTO then takes the mailbox --
// instead of in the middle of somebody's alignment.
int exchange_handshake_rccl(oa_ctx *p)
{
    Exchange *x = p->xch;
    const size_t n = p->subs.size();
    std::vector<double *> bufs(n, nullptr);
    int rc = OA_OK;
    const int keep_mode = x->mode;
    for (size_t i = 0; i < n && !rc; ++i) {
        oa_ctx *c = p->subs[i];
        if ((rc = use_device(c))) break;
        double h[oa::NSUMS];
        for (int k = 0; k < oa::NSUMS; ++k) h[k] = (double)(i + 1) * (k + 1);
        hipError_t e = hipMalloc((void **)&bufs[i], sizeof h);
        if (e == hipSuccess) e = hipMemcpy(bufs[i], h, sizeof h, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail(OA_E_HIP, "RCCL handshake: %s", hipGetErrorString(e));
    }
    if (!rc) {
        ncclResult_t r = x->GroupStart();
        for (size_t i = 0; i < n && r == ncclSuccess; ++i) {
            oa_ctx *c = p->subs[i];
            if (hipSetDevice(c->device) != hipSuccess) { r = (ncclResult_t)1; break; }
            r = x->AllReduce(bufs[i], bufs[i], oa::NSUMS, ncclDouble, ncclSum, x->comms[i], c->stream);
        }
        const ncclResult_t r2 = x->GroupEnd();
        if (r == ncclSuccess) r = r2;
        if (r != ncclSuccess) rc = fail(OA_E_RCCL, "RCCL handshake: ncclAllReduce failed: %s", x->GetErrorString ? x->GetErrorString(r) : "?");
    }
    if (!rc) {
        x->mode = OA_EXCHANGE_RCCL;                                     // (multi_wait's watchdog is the RCCL one)
        rc = multi_wait(p, false, false);
        x->mode = keep_mode;
    }
    for (size_t i = 0; i < n && !rc; ++i) {
        double h[oa::NSUMS];
        if (hipSetDevice(p->subs[i]->device) != hipSuccess || hipMemcpy(h, bufs[i], sizeof h, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(OA_E_HIP, "RCCL handshake: read-back failed"); break; }
        for (int k = 0; k < oa::NSUMS; ++k)
            if (h[k] != (double)(n * (n + 1) / 2) * (k + 1)) { rc = fail(OA_E_RCCL, "RCCL handshake: device %d holds a wrong sum", p->subs[i]->device); break; }
    }
    for (size_t i = 0; i < n; ++i) if (bufs[i]) { (void)hipSetDevice(p->subs[i]->device); (void)hipFree(bufs[i]); }
    if (rc && !x->comms.empty()) { const std::string keep = g_err; exchange_abort_rccl(p, "handshake failed"); g_err = keep; }
    if (!rc) { x->rccl_aborted = false; x->rccl_ranks_last = (int)n; }
    return rc;
}

int exchange_init_rccl(oa_ctx *p)
{
    Exchange *x = p->xch;
    if (!x->comms.empty()) return OA_OK;
    for (size_t i = 0; i < p->subs.size(); ++i)
        for (size_t j = 0; j < i; ++j)
            if (p->subs[i]->device == p->subs[j]->device)
                return fail(OA_E_RCCL, "OA_EXCHANGE_RCCL needs distinct devices (device %d is listed twice); use OA_EXCHANGE_MAILBOX", p->subs[i]->device);
    if (!x->lib) {
        const char *names[] = { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" };
        for (const char *nm : names) if ((x->lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL))) break;
        if (!x->lib) return fail(OA_E_RCCL, "librccl not found (%s)", dlerror());
        x->CommInitAll = (decltype(x->CommInitAll))dlsym(x->lib, "ncclCommInitAll");
        x->CommDestroy = (decltype(x->CommDestroy))dlsym(x->lib, "ncclCommDestroy");
        x->CommCount = (decltype(x->CommCount))dlsym(x->lib, "ncclCommCount");
        x->AllReduce = (decltype(x->AllReduce))dlsym(x->lib, "ncclAllReduce");
        x->GroupStart = (decltype(x->GroupStart))dlsym(x->lib, "ncclGroupStart");
        x->GroupEnd = (decltype(x->GroupEnd))dlsym(x->lib, "ncclGroupEnd");
        x->GetErrorString = (decltype(x->GetErrorString))dlsym(x->lib, "ncclGetErrorString");
        x->CommAbort = (decltype(x->CommAbort))dlsym(x->lib, "ncclCommAbort");
        x->CommGetAsyncError = (decltype(x->CommGetAsyncError))dlsym(x->lib, "ncclCommGetAsyncError");
        if (!x->CommInitAll || !x->CommDestroy || !x->AllReduce || !x->GroupStart || !x->GroupEnd || !x->CommAbort)
            return fail(OA_E_RCCL, "librccl lacks the expected entry points");
    }
    std::vector<int> devs;
    for (oa_ctx *c : p->subs) devs.push_back(c->device);
    x->comms.assign(devs.size(), nullptr);
    ncclResult_t r = x->CommInitAll(x->comms.data(), (int)devs.size(), devs.data());
    if (r != ncclSuccess) {
        x->comms.clear();
        return fail(OA_E_RCCL, "ncclCommInitAll failed: %s", x->GetErrorString ? x->GetErrorString(r) : "?");
    }
    return exchange_handshake_rccl(p);
}

// how many ranks RCCL's communicator spans (0 = RCCL is not what this context exchanges through)
int exchange_rccl_ranks(const Exchange *x)
{
    if (!x || x->mode != OA_EXCHANGE_RCCL || x->comms.empty()) return 0;
    int n = 0;
    if (x->CommCount && x->CommCount(x->comms[0], &n) == ncclSuccess) return n;
    return (int)x->comms.size();
}

// AUTO -> RCCL when the devices are distinct and RCCL comes up, else the mailbox.  Decided once, before the first loop
// (ncclCommInitAll takes ~0.1-1 s: not something to pay inside oa_create_multi for contexts that only upload and pair).
int exchange_resolve(oa_ctx *p)
{
    Exchange *x = p->xch;
    if (x->resolved) return OA_OK;
    if (x->requested == OA_EXCHANGE_RCCL) {
        const int rc = exchange_init_rccl(p);
        if (rc) return rc;
        x->mode = OA_EXCHANGE_RCCL;
    } else if (x->requested == OA_EXCHANGE_MAILBOX) {
        x->mode = OA_EXCHANGE_MAILBOX;
    } else {
        x->mode = OA_EXCHANGE_MAILBOX;
        const bool any = p->tune.auto_rccl_any;                // test hook: AUTO takes RCCL for a world of one too (the fallback of multi_run on a one-GPU box)
        if (p->subs.size() < 2 && !any) x->auto_note = "one device: nothing to exchange";
        else if (!devices_distinct(p)) x->auto_note = "a device is listed more than once";
        else if (x->rccl_aborted) { /* auto_note says why: a communicator that hung once is not trusted again unasked */ }
        else {
            const std::string keep = g_err;
            if (exchange_init_rccl(p) == OA_OK) x->mode = OA_EXCHANGE_RCCL;
            else { x->auto_note = g_err; g_err = keep; }
        }
    }
    if (x->mode == OA_EXCHANGE_RCCL) x->agree_on = true;             // the test hook that switches the agreement off is for the mailbox only
    x->resolved = true;
    return OA_OK;
}

void exchange_destroy(oa_ctx *p)
{
    Exchange *x = p->xch;
    if (!x) return;
    for (ncclComm_t cm : x->comms) if (cm && x->CommDestroy) (void)x->CommDestroy(cm);
    for (size_t r = 0; r < p->subs.size(); ++r) {
        if (hipSetDevice(p->subs[r]->device) != hipSuccess) { (void)hipGetLastError(); continue; }
        if (r < x->d_dests.size() && x->d_dests[r]) (void)hipFree(x->d_dests[r]);
        if (x->device_box && r < x->box.size() && x->box[r]) (void)hipFree(x->box[r]);
    }
    if (x->h_box) (void)hipHostFree(x->h_box);
    if (x->h_release) (void)hipHostFree(x->h_release);
    // the library handle stays open: unloading RCCL under a live HIP runtime is not worth the risk
    delete x;
    p->xch = nullptr;
}

// Mailboxes of a new multi-device context.  Device placement needs every pair of distinct devices to map each other's
// memory (hipDeviceEnablePeerAccess) and a fine-grained allocation per rank; anything less falls back to the pinned host
// box.  OA_MAILBOX=host / device forces one (device: fails instead of falling back).
int exchange_setup_mailboxes(oa_ctx *p)
{
    Exchange *x = p->xch;
    const int world = x->world;
    const size_t bytes = sizeof(oa::MailSlot) * 2 * (size_t)world;
    const bool force_host = p->tune.mailbox == 1, force_dev = p->tune.mailbox == 2;
    bool dev_ok = !force_host;
    std::string why;
    if (dev_ok) {
        for (int i = 0; i < world && dev_ok; ++i)
            for (int j = 0; j < world && dev_ok; ++j) {
                const int di = p->subs[(size_t)i]->device, dj = p->subs[(size_t)j]->device;
                if (di == dj) continue;
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, di, dj) != hipSuccess || !can) { (void)hipGetLastError(); dev_ok = false; why = "no peer access between the listed devices"; break; }
                if (hipSetDevice(di) != hipSuccess) { (void)hipGetLastError(); dev_ok = false; why = "hipSetDevice failed"; break; }
                const hipError_t e = hipDeviceEnablePeerAccess(dj, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { dev_ok = false; why = std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e); }
                (void)hipGetLastError();
            }
    }
    x->box.assign((size_t)world, nullptr);
    x->d_dests.assign((size_t)world, nullptr);
    if (dev_ok) {
        for (int r = 0; r < world && dev_ok; ++r) {
            void *ptr = nullptr;
            hipError_t e = hipSetDevice(p->subs[(size_t)r]->device);
            if (e == hipSuccess) e = hipExtMallocWithFlags(&ptr, bytes, hipDeviceMallocFinegrained);
            if (e == hipSuccess) e = hipMemset(ptr, 0, bytes);
            if (e != hipSuccess) { (void)hipGetLastError(); dev_ok = false; why = std::string("fine-grained device allocation: ") + hipGetErrorString(e); if (ptr) (void)hipFree(ptr); break; }
            x->box[(size_t)r] = (oa::MailSlot *)ptr;
        }
        if (!dev_ok) for (int r = 0; r < world; ++r) if (x->box[(size_t)r]) { (void)hipSetDevice(p->subs[(size_t)r]->device); (void)hipFree(x->box[(size_t)r]); x->box[(size_t)r] = nullptr; }
    }
    if (!dev_ok && force_dev) return fail(OA_E_HIP, "OA_MAILBOX=device: %s", why.c_str());
    x->device_box = dev_ok;
    if (!dev_ok) {
        hipError_t e = hipHostMalloc((void **)&x->h_box, bytes, hipHostMallocPortable | hipHostMallocMapped);
        if (e != hipSuccess) return fail(OA_E_HIP, "oa_create_multi: mailbox allocation failed: %s", hipGetErrorString(e));
        memset(x->h_box, 0, bytes);
        for (int r = 0; r < world; ++r) {
            void *dp = nullptr;
            e = hipSetDevice(p->subs[(size_t)r]->device);
            if (e == hipSuccess) e = hipHostGetDevicePointer(&dp, x->h_box, 0);
            if (e != hipSuccess) return fail(OA_E_HIP, "oa_create_multi: device %d cannot map the mailbox: %s", p->subs[(size_t)r]->device, hipGetErrorString(e));
            x->box[(size_t)r] = (oa::MailSlot *)dp;
        }
    }
    // where rank r posts: every rank's inbox (device placement) or the one host box as r's device sees it
    x->n_dest = dev_ok ? world : 1;
    for (int r = 0; r < world; ++r) {
        std::vector<oa::MailSlot *> dst;
        if (dev_ok) dst = x->box; else dst.push_back(x->box[(size_t)r]);
        void *dp = nullptr;
        hipError_t e = hipSetDevice(p->subs[(size_t)r]->device);
        if (e == hipSuccess) e = hipMalloc(&dp, sizeof(oa::MailSlot *) * dst.size());
        if (e == hipSuccess) e = hipMemcpy(dp, dst.data(), sizeof(oa::MailSlot *) * dst.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(OA_E_HIP, "oa_create_multi: mailbox table: %s", hipGetErrorString(e));
        x->d_dests[(size_t)r] = (oa::MailSlot **)dp;
    }
    return OA_OK;
}

// One iteration on the children of one host thread's group: pass 1 search + accumulate + post / reduce on each child,
// [all-reduce], pass 2 gather + solve on each.  (Two passes, not child by child: children that share a GPU may share a
// hardware queue, and every post of an iteration has to be submitted ahead of the gathers that wait for it.)
int multi_iteration_group(oa_ctx *p, const std::vector<int> &group, bool timed)
{
    Exchange *x = p->xch;
    int rc;
    const auto t0 = std::chrono::steady_clock::now();
    for (int i : group) {
        oa_ctx *c = p->subs[(size_t)i];
        if ((rc = use_device(c))) return rc;
        oa::RowSel sel;
        bool fused;
        if ((rc = launch_search_accumulate(c, timed, sel, fused))) return rc;
        if (x->mode == OA_EXCHANGE_RCCL) rc = launch_reduce(c, c->d_sums, sel, fused);
        else {
            hipLaunchKernelGGL(oa::k_reduce_post, dim3(1), dim3(oa::RED_THREADS), 0, c->stream, (const oa::DevState *)c->d_state,
                               (const double *)c->d_partials, sel,
                               (oa::MailSlot *const *)x->d_dests[(size_t)c->rank], x->n_dest, c->rank, x->world,
                               x->fault_skip_rank == c->rank ? 1 : 0, fused ? &c->d_state->t_acc_start : (unsigned long long *)nullptr);
            HIPCHK(hipGetLastError());
        }
        if (rc) return rc;
    }
    if (x->mode == OA_EXCHANGE_RCCL) {
        if (x->comms.empty()) return fail(OA_E_RCCL, "multi-device exchange: the RCCL communicators were aborted");
        // (test hook: this rank's stream stops here, ahead of its collective, until the watchdog releases it -- what a rank
        //  whose peers never enter the collective looks like to the host; bounded, so that a test can never hang the GPU)
        for (int i : group) {
            oa_ctx *c = p->subs[(size_t)i];
            if (c->rank == x->fault_stall_rank.load(std::memory_order_relaxed) && c->enq_iters == x->fault_stall_iter && x->h_release) {
                if ((rc = use_device(c))) return rc;
                void *dp = nullptr;
                HIPCHK(hipHostGetDevicePointer(&dp, x->h_release, 0));
                hipLaunchKernelGGL(oa::k_fault_stall, dim3(1), dim3(64), 0, c->stream, (const int32_t *)dp, (unsigned long long)(20.0 * c->wall_clock_khz * 1e3));
                HIPCHK(hipGetLastError());
                x->fault_stall_rank.store(-1, std::memory_order_relaxed);   // once
            }
        }
        // one thread, several devices: group semantics; one thread per device: plain calls (each rank's kernel waits
        // for its peers on the device, the host call only enqueues)
        const bool grouped = group.size() > 1;
        if (grouped) RCCLCHK(x, x->GroupStart());
        for (int i : group) {
            oa_ctx *c = p->subs[(size_t)i];
            if ((rc = use_device(c))) { if (grouped) (void)x->GroupEnd(); return rc; }
            ncclResult_t r = x->AllReduce(c->d_sums, c->d_sums, oa::NSUMS, ncclDouble, ncclSum, x->comms[(size_t)i], c->stream);
            if (r != ncclSuccess) { if (grouped) (void)x->GroupEnd(); return fail(OA_E_RCCL, "ncclAllReduce failed: %s", x->GetErrorString ? x->GetErrorString(r) : "?"); }
        }
        if (grouped) RCCLCHK(x, x->GroupEnd());
    }
    for (int i : group) {
        oa_ctx *c = p->subs[(size_t)i];
        if ((rc = use_device(c))) return rc;
        if (x->mode == OA_EXCHANGE_RCCL) rc = iter_finish(c, c->d_sums);
        else {
            hipLaunchKernelGGL(oa::k_gather_solve_update, dim3(1), dim3(128), 0, c->stream, c->d_state, x->box[(size_t)c->rank],
                               x->world, c->d_sums, c->d_hist, c->src.d_todo_count, x->timeout_ticks);
            HIPCHK(hipGetLastError());
        }
        if (rc) return rc;
    }
    const double ns = (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    for (int i : group) { p->subs[(size_t)i]->enq_ns += ns / (double)group.size(); p->subs[(size_t)i]->enq_iters++; }
    return OA_OK;
}

// f(group index) on every host thread of the context (group 0 on the caller's)
template <typename F> int multi_for_groups(oa_ctx *p, F f)
{
    if (p->groups.size() <= 1 || !p->pool) {
        for (size_t g = 0; g < p->groups.size(); ++g) { const int rc = f(g); if (rc) return rc; }
        return OA_OK;
    }
    return p->pool->run(p->groups.size(), f);
}

// end whatever loop is open: wait for the streams (bounded, see multi_wait), close the loop on every child.
// failed: a host thread gave up in the middle of enqueuing -- in RCCL mode the ranks' collective counts may differ
void multi_abort(oa_ctx *p, bool failed = false)
{
    const std::string keep = g_err;
    (void)multi_wait(p, failed && p->xch && p->xch->mode == OA_EXCHANGE_RCCL && p->loop_active);
    g_err = keep;
    for (oa_ctx *c : p->subs) c->loop_active = false;
    p->loop_active = false;
}

int multi_begin(oa_ctx *p, const oa_settings *st, int iters)
{
    Exchange *x = p->xch;
    int rc;
    if ((rc = exchange_resolve(p))) return rc;
    // sequence numbers of this loop's posts: above everything an earlier loop left in the mailboxes
    const unsigned long long seq_base = x->seq_next;
    x->seq_next += (iters == ITERATE_OPEN || iters < 0) ? (1ull << 32) : (unsigned long long)iters + 2ull;
    for (oa_ctx *c : p->subs) {
        c->h_state.seq_base = seq_base;
        if ((rc = begin_loop(c, st, iters))) { multi_abort(p); return rc; }     // synchronises the child's stream first
        if ((rc = ensure_events(c, (c->time_events && iters != ITERATE_OPEN) ? std::max(1, std::min(iters, 1 << 16)) : 1))) { multi_abort(p); return rc; }
        c->enq_ns = 0.0; c->enq_iters = 0;
    }
    for (oa_ctx *c : p->subs) {
        if ((rc = use_device(c))) { multi_abort(p); return rc; }
        HIPCHK(hipEventRecord(c->ev_loop0, c->stream));
    }
    x->agree_committed = 0;
    x->agree_stop_at.store(-1);
    if (x->h_release) __atomic_store_n(x->h_release, 0, __ATOMIC_RELEASE);
    p->settings = *st;
    p->loop_active = true;
    return OA_OK;
}

int status_error(int status)
{
    if (status == OA_E_TOO_FEW_PAIRS) return fail(OA_E_TOO_FEW_PAIRS, "input arrays are of wrong shape or type");
    if (status == OA_E_SINGULAR) return fail(OA_E_SINGULAR, "align matrix_world became singular");
    if (status == OA_E_RCCL) return fail(OA_E_RCCL, "multi-device exchange: a device's sums did not arrive in time");
    return OA_OK;
}

int multi_end(oa_ctx *p, oa_report *rep)
{
    int rc = OA_OK;
    oa_report agg{};
    for (oa_ctx *c : p->subs) {
        if ((rc = use_device(c))) break;
        if (hipEventRecord(c->ev_loop1, c->stream) != hipSuccess) { rc = fail(OA_E_HIP, "hipEventRecord failed"); break; }
    }
    if (!rc) rc = multi_wait(p);                                   // bounded in RCCL mode: a hung collective becomes OA_E_RCCL
    if (rc) { for (oa_ctx *c : p->subs) c->loop_active = false; p->loop_active = false; return rc; }
    for (size_t i = 0; i < p->subs.size(); ++i) {
        oa_ctx *c = p->subs[i];
        oa_report r{};
        int rci = use_device(c);
        if (!rci) rci = fill_report(c, &r);
        float ms = 0.f;
        if (!rci && hipEventElapsedTime(&ms, c->ev_loop0, c->ev_loop1) == hipSuccess) r.loop_ms = ms;
        c->loop_active = false;
        if (rci) { if (!rc) rc = rci; continue; }
        c->last_nn_ms = r.nn_ms_total;
        if (i == 0) agg = r;
        else {
            agg.nn_ms_total = std::max(agg.nn_ms_total, r.nn_ms_total);      // the slowest device sets the pace
            agg.loop_ms = std::max(agg.loop_ms, r.loop_ms);
            if (agg.status == 0 && r.status != 0) agg.status = r.status;
        }
    }
    p->loop_active = false;
    if (rc) return rc;
    *rep = agg;
    return status_error(agg.status);
}

// May this host thread enqueue iteration `it`?  halt_seen: its own device has reported the halt.  See Exchange::agree_mu.
bool agree_next(Exchange *x, int it, bool halt_seen)
{
    if (!x->agree_on) return !halt_seen;
    std::lock_guard<std::mutex> lk(x->agree_mu);
    int stop = x->agree_stop_at.load(std::memory_order_relaxed);
    if (stop < 0 && halt_seen) { stop = x->agree_committed; x->agree_stop_at.store(stop, std::memory_order_release); }
    if (stop >= 0) return it < stop;
    x->agree_committed = std::max(x->agree_committed, it + 1);
    return true;
}

// a host thread failed: nobody commits to anything new (the failing thread's own count is whatever it got to -- multi_run
// then aborts the communicators instead of waiting for collectives that cannot complete)
void agree_fail(Exchange *x)
{
    std::lock_guard<std::mutex> lk(x->agree_mu);
    if (x->agree_stop_at.load(std::memory_order_relaxed) < 0) x->agree_stop_at.store(x->agree_committed, std::memory_order_release);
}

// the loop of one host thread's group: enqueue its children's iterations, at most `lag` ahead of the GPU, until the
// budget is spent or the threads have agreed on where the loop ends (every device takes the same decision from the same
// sums, but the threads hear of it at different times: agree_next)
int multi_group_loop(oa_ctx *p, size_t g, const oa_settings *st)
{
    const std::vector<int> &group = p->groups[g];
    if (group.empty()) return OA_OK;
    Exchange *x = p->xch;
    oa_ctx *c0 = p->subs[(size_t)group[0]];
    // (the adaptive grid path needs recent news from the device too: then the host stays close even without early exit)
    bool poll = loop_polls(c0, st);
    const int lag = 2;
    volatile int32_t *progress = c0->h_poll;
    for (int it = 0; it < st->iters; ++it) {
        bool halt_seen = false;
        if (poll) {                                                     // see oa_run
            const auto t_wait = std::chrono::steady_clock::now();
            while (!progress[0] && progress[1] < it - lag && x->agree_stop_at.load(std::memory_order_acquire) < 0) {
                if (std::chrono::steady_clock::now() - t_wait > std::chrono::seconds(5)) { poll = false; break; }   // once is enough: enqueue the rest blindly
                std::this_thread::yield();
            }
            if ((int)g == x->fault_lag_group && x->fault_lag_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(x->fault_lag_us));
            halt_seen = progress[0] != 0;
        }
        if (!agree_next(x, it, halt_seen)) break;
        int rc = OA_OK;
        if (it == x->fault_fail_iter) {
            int want = (int)g;
            if (x->fault_fail_group.compare_exchange_strong(want, -1)) rc = fail(OA_E_HIP, "injected enqueue failure (OA_FAULT_FAIL_GROUP)");   // once
        }
        if (!rc) rc = multi_iteration_group(p, group, true);
        if (rc) { agree_fail(x); return rc; }
    }
    return OA_OK;
}

int multi_run(oa_ctx *p, const oa_settings *st, oa_report *rep)
{
    for (int attempt = 0;; ++attempt) {
        int rc = multi_begin(p, st, st->iters);
        if (rc) return rc;
        const bool was_rccl = p->xch && p->xch->mode == OA_EXCHANGE_RCCL;
        rc = multi_for_groups(p, [p, st](size_t g) -> int { return multi_group_loop(p, g, st); });
        const bool enqueued = rc == OA_OK;
        if (enqueued) rc = multi_end(p, rep);                       // (waits: the watchdog's OA_E_RCCL comes out of here)
        if (!rc) return OA_OK;
        const std::string keep = g_err;
        if (!enqueued) multi_abort(p, true);
        // AUTO had picked RCCL and RCCL let the loop down (watchdog, asynchronous error: the communicators are aborted and AUTO
        // resolves to the mailboxes from here on): the caller asked for an alignment, not for RCCL -- the same loop once more,
        // through the mailboxes.  The children's host mirrors still hold the pose the loop started from (a loop's state comes
        // back to the host in multi_end only); what the failed attempt left on the devices -- seeds -- changes no result.
        // An explicit oa_set_exchange(RCCL) gets the error.  (the RCCL path has never run on distinct GPUs.)
        if (rc == OA_E_RCCL && attempt == 0 && was_rccl && p->xch->requested == OA_EXCHANGE_AUTO && p->xch->rccl_aborted) {
            p->xch->rccl_fallbacks++;
            if (!p->subs.empty() && p->subs[0]->tune.debug) fprintf(stderr, "[oa] RCCL failed (%s): the loop runs again through the mailboxes\n", keep.c_str());
            continue;
        }
        g_err = keep;
        return rc;
    }
}
}  // namespace

// ================================================================================================
// lifetime
// ================================================================================================
OA_EXPORT const char *oa_last_error(void) { return g_err.c_str(); }
OA_EXPORT const char *oa_version(void) { return "oa_icp 0.1 (gfx950)"; }

OA_EXPORT int oa_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

OA_EXPORT int oa_create(oa_ctx **out, int device)
{
    if (!out) return fail(OA_E_BAD_ARG, "oa_create: null out pointer");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(OA_E_NO_DEVICE, "no HIP device available: the oa_icp engine has no CPU fallback");
    }
    if (device < 0 || device >= n) return fail(OA_E_BAD_ARG, "device %d out of range (0..%d)", device, n - 1);
    oa_ctx *c = new (std::nothrow) oa_ctx();
    if (!c) return fail(OA_E_HIP, "out of host memory");
    c->device = device;
    memset(&c->h_state, 0, sizeof c->h_state);
    memset(&c->settings, 0, sizeof c->settings);
    hipError_t e = hipSetDevice(device);
    hipDeviceProp_t prop;
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) { c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256; }
    if (e == hipSuccess) {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) c->wall_clock_khz = (double)khz;
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(OA_E_HIP, "oa_create: %s", hipGetErrorString(e)); }
    c->stream = c->own_stream;
    c->src.R = c->tune.nn_r ? c->tune.nn_r : 4;
    c->grid_mode = c->tune.nn_grid;
    dev_cache().context_created();
    *out = c;
    return OA_OK;
}

// oa_create(&ctx, devices, n_dev).  One process, one child context (and stream) per listed device; the
// same device may be listed more than once -- that is how the multi-device path is tested on a single GPU.  Children
// that share a device share one stream by default (the exchange's waits then can never sit in front of the post they
// wait for); OA_MULTI_OWN_STREAMS=1 gives each its own, so that k_gather_solve_update really spins against concurrent
// producers on a one-GPU box (the two-pass enqueue order of multi_iteration_group keeps that deadlock-free).
OA_EXPORT int oa_create_multi(oa_ctx **out, const int *devices, int n_dev)
{
    if (!out) return fail(OA_E_BAD_ARG, "oa_create_multi: null out pointer");
    *out = nullptr;
    if (!devices || n_dev < 1 || n_dev > 64) return fail(OA_E_BAD_ARG, "oa_create_multi: 1..64 devices, got %d", n_dev);
    oa_ctx *p = new (std::nothrow) oa_ctx();
    if (!p) return fail(OA_E_HIP, "out of host memory");
    memset(&p->h_state, 0, sizeof p->h_state);
    memset(&p->settings, 0, sizeof p->settings);
    p->device = devices[0];
    p->world = n_dev;
    Exchange *x = new (std::nothrow) Exchange();
    if (!x) { delete p; return fail(OA_E_HIP, "out of host memory"); }
    p->xch = x;
    x->world = n_dev;
    const bool own_streams = p->tune.multi_own_streams;
    int rc = OA_OK;
    for (int i = 0; i < n_dev && !rc; ++i) {
        oa_ctx *c = nullptr;
        rc = oa_create(&c, devices[i]);
        if (rc) break;
        c->parent = p; c->rank = i; c->world = n_dev; c->xch = x;
        if (!own_streams)
            for (oa_ctx *e : p->subs) if (e->device == c->device) { c->stream = e->stream; break; }   // one stream per device
        p->subs.push_back(c);
    }
    if (!rc) rc = exchange_setup_mailboxes(p);
    if (!rc) {
        const double secs = p->tune.exchange_timeout_s;
        x->timeout_ticks = (unsigned long long)(secs * p->subs[0]->wall_clock_khz * 1e3);
        x->seq_next = 0;
        x->timeout_s = secs;
        x->fault_skip_rank = p->tune.fault_skip_post_rank;
        x->agree_on = p->tune.multi_agree;
        x->fault_lag_group = p->tune.fault_lag_group;
        x->fault_lag_us = p->tune.fault_lag_us;
        x->fault_fail_group.store(p->tune.fault_fail_group);
        x->fault_fail_iter = p->tune.fault_fail_iter;
        x->fault_stall_rank.store(p->tune.fault_stall_rank);
        x->fault_stall_iter = p->tune.fault_stall_iter;
        if (x->fault_stall_rank.load() >= 0) {
            if (hipHostMalloc((void **)&x->h_release, sizeof(int32_t), hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); x->h_release = nullptr; }
            else *x->h_release = 0;
        }
        static_assert(OA_EXCHANGE_AUTO == -1 && OA_EXCHANGE_MAILBOX == 0 && OA_EXCHANGE_RCCL == 1, "Tunables::exchange holds these values");
        x->requested = p->tune.exchange;
        // host threads: one group of children per GPU (OA_MULTI_THREADS=1: per child, 0: a single group).  In the loop
        // children that share a STREAM always share a thread: enqueued from two threads, one child's gather could land
        // in front of the post it waits for.
        const int threads = p->tune.multi_threads;
        auto deal = [&](std::vector<std::vector<int>> &groups, bool per_child) {
            for (int i = 0; i < n_dev; ++i) {
                size_t g = groups.size();
                if (threads == 0) g = 0;
                else if (!per_child)
                    for (size_t k = 0; k < groups.size(); ++k)
                        if (p->subs[(size_t)groups[k][0]]->device == devices[i]) { g = k; break; }
                if (g == groups.size()) groups.emplace_back();
                groups[g].push_back(i);
            }
        };
        // (per-child loop threads only while the children of a GPU fit its hardware queues -- HIP multiplexes streams
        //  over 4 of them -- or two children's packets can end up in one queue in the wrong order; a test-box matter:
        //  on distinct GPUs every child has a device of its own)
        int max_on_one = 0;
        for (int i = 0; i < n_dev; ++i) {
            int same = 0;
            for (int j = 0; j < n_dev; ++j) same += devices[j] == devices[i] ? 1 : 0;
            max_on_one = std::max(max_on_one, same);
        }
        deal(p->upload_groups, threads > 0);
        deal(p->groups, threads > 0 && own_streams && max_on_one <= 4);
        const size_t n_threads = std::max(p->groups.size(), p->upload_groups.size());
        if (n_threads > 1) {
            p->pool = new (std::nothrow) WorkerPool();
            if (!p->pool) rc = fail(OA_E_HIP, "out of host memory");
            else p->pool->start(n_threads - 1);
        }
    }
    if (rc) { const std::string keep = g_err; oa_destroy(p); g_err = keep; return rc; }
    *out = p;
    return OA_OK;
}

OA_EXPORT int oa_set_exchange(oa_ctx *c, int mode)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (c->subs.empty()) return fail(OA_E_STATE, "oa_set_exchange: not a multi-device context (oa_create_multi)");
    if (mode != OA_EXCHANGE_AUTO && mode != OA_EXCHANGE_MAILBOX && mode != OA_EXCHANGE_RCCL) return fail(OA_E_BAD_ARG, "exchange mode %d", mode);
    if (c->loop_active) multi_abort(c);                                 // an open oa_iterate sequence ends here
    c->xch->requested = mode;
    c->xch->resolved = false;
    return exchange_resolve(c);                                         // RCCL fails now rather than in the first iteration
}

// why the exchange is what it is: the reason AUTO did not take (or no longer takes) RCCL -- "a device is listed more than once",
// librccl's load error, "RCCL was aborted: ..." after a watchdog abort -- or "" when there is nothing to say
OA_EXPORT const char *oa_exchange_note(oa_ctx *c)
{
    static thread_local std::string note;
    note = (c && c->xch) ? c->xch->auto_note : std::string();
    return note.c_str();
}

OA_EXPORT int oa_num_devices(oa_ctx *c) { return !c ? 0 : (c->subs.empty() ? 1 : (int)c->subs.size()); }

OA_EXPORT void oa_release_cached_memory(void) { dev_cache().trim(0, 0); }

OA_EXPORT void oa_destroy(oa_ctx *c)
{
    if (!c) return;
    if (!c->subs.empty() || c->xch) {
        if (!c->parent) {                                           // a multi-device parent: workers, exchange, then the children
            for (oa_ctx *sub : c->subs) { if (hipSetDevice(sub->device) == hipSuccess) (void)hipStreamSynchronize(sub->stream); }
            delete c->pool;
            c->pool = nullptr;
            exchange_destroy(c);
            for (oa_ctx *sub : c->subs) { sub->xch = nullptr; sub->parent = nullptr; oa_destroy(sub); }
            delete c;
            return;
        }
    }
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    tl_stream_known = false;                                        // the stream below is about to go away
    const oa::DevTeardown settled;                                  // the device is idle: `delete c` hands every block back without a synchronisation each
    if (c->h_hist_map) (void)hipHostFree(c->h_hist_map);
    if (c->h_state_pin) (void)hipHostFree(c->h_state_pin);
    if (c->h_scratch) (void)hipHostFree(c->h_scratch);
    if (c->h_result) (void)hipHostFree(c->h_result);
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    if (c->ev_loop0) (void)hipEventDestroy(c->ev_loop0);
    if (c->h_poll) (void)hipHostFree(c->h_poll);
    if (c->ev_loop1) (void)hipEventDestroy(c->ev_loop1);
    if (c->own_stream) { dev_cache().stream_gone(c->own_stream); (void)hipStreamDestroy(c->own_stream); }
    delete c;
    dev_cache().context_destroyed();                                // the last context gives the cached blocks back
}

OA_EXPORT int oa_set_search_mode(oa_ctx *c, int mode)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (mode < -1 || mode > 2) return fail(OA_E_BAD_ARG, "search mode %d (use OA_SEARCH_AUTO/BRUTE/GRID/BVH)", mode);
    OA_ROUTE_ALL(c, oa_set_search_mode(sub, mode));
    const bool rebuild = (c->grid_mode == 0 && mode != 0 && c->tgt.nt > 0);
    const bool sorted_now = (mode == 0 && c->tgt.nt > 0 && !c->tgt.surface && !c->tgt.d_tfs);   // (skipped when the target was uploaded)
    c->grid_mode = mode;
    if (sorted_now) {
        int rc = use_device(c);
        if (rc) return rc;
        if ((rc = build_sorted_images(c))) return rc;
    }
    if (mode == 0 && c->src.ns_pad > 0 && c->src.d_src4) {                  // (a source uploaded for the other modes: what source_reset allocates for this one)
        int rc = use_device(c);
        if (rc) return rc;
        if ((rc = ensure_sorted_buffers(c, c->src.ns_pad / (oa::NN_THREADS * c->src.R)))) return rc;
    }
    if (rebuild) {                                   // the grids were skipped when the target was uploaded
        int rc = use_device(c);
        if (rc) return rc;
        if (!c->tgt.grid_ok && (rc = build_grid(c))) return rc;
        if (!c->tgt.bvh_ok && (rc = build_bvh(c, false))) return rc;
        if (c->tgt.surface && !c->tgt.tri_grid_ok && (rc = build_tri_grid(c))) return rc;
        if (c->tgt.surface && !c->tgt.tbvh_ok && (rc = build_bvh(c, true))) return rc;
    }
    return OA_OK;
}

OA_EXPORT int oa_set_stream(oa_ctx *c, void *stream)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (!c->subs.empty())
        return stream == OA_STREAM_OWN ? OA_OK : fail(OA_E_STATE, "oa_set_stream: a multi-device context runs on its own streams (one per device)");
    if (c->parent && stream != OA_STREAM_OWN) return fail(OA_E_STATE, "oa_set_stream: child of a multi-device context");
    // the handle is used as given: NULL is HIP's legacy default stream (what torch.cuda.current_stream() is
    // unless the caller switched streams); OA_STREAM_OWN selects the context's private non-blocking stream
    c->stream = (stream == OA_STREAM_OWN) ? c->own_stream : (hipStream_t)stream;
    return OA_OK;
}

// ================================================================================================
// uploads
// ================================================================================================
namespace {
// nb x 6 bounding-box partials of a float[3n] array, on the host (the stream has been waited for on return)
int bbox_partials(oa_ctx *c, const float *d_xyz, long long n, int nb, float *out)
{
    void *dv; const void *hv;
    int rc = result_buffer(c, sizeof(float) * 6 * (size_t)nb, &dv, &hv);
    if (rc) return rc;
    if (dv) {
        hipLaunchKernelGGL(oa::k_bbox_partial, dim3(nb), dim3(256), 0, c->stream, d_xyz, (int)n, (float *)dv);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));
        memcpy(out, hv, sizeof(float) * 6 * (size_t)nb);
        return OA_OK;
    }
    DevTmp<float> d_bb;
    HIPCHK(d_bb.alloc(6 * (size_t)nb));
    hipLaunchKernelGGL(oa::k_bbox_partial, dim3(nb), dim3(256), 0, c->stream, d_xyz, (int)n, d_bb.p);
    HIPCHK(hipGetLastError());
    return read_small(c, out, d_bb, sizeof(float) * 6 * (size_t)nb);
}
// nb rows of {lo[3], hi[3]} (k_bbox_partial, k_bbox_finite, k_voxel_bbox) folded in row order -> lo / hi; true if an entry is NaN.
// No row, or none that compares: lo = +inf, hi = -inf.  What an empty box or a NaN means is the caller's to say.
bool fold_bbox(const float *bb, int nb, float lo[3], float hi[3])
{
    bool any_nan = false;
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (int b = 0; b < nb; ++b)
        for (int a = 0; a < 3; ++a) {
            const float l = bb[6 * (size_t)b + a], h = bb[6 * (size_t)b + 3 + a];
            if (l != l || h != h) any_nan = true;
            if (l < lo[a]) lo[a] = l;
            if (h > hi[a]) hi[a] = h;
        }
    return any_nan;
}

// filter image for k_nn_search_filtered: bbox centre, centred -2q / |q|^2 arrays, max |q - centre|
// k_nn_search_sorted's images: the target in the order of its coordinate along the longest axis (30-bit quantised key through
// the library's stable argsort -- the order is for speed only, any permutation gives the same answers).  Needs build_filter's
// results (bounding box, centre, axes, filter_ok); allocates, so it runs with the upload or from oa_set_search_mode, never
// inside a loop.
int build_sorted_images(oa_ctx *c)
{
    c->tgt.d_tfs.reset(); c->tgt.d_tf3s.reset(); c->tgt.d_tgs.reset(); c->tgt.d_tmw.reset(); c->tgt.d_toct.reset(); c->tgt.oct_c = 0.0f; c->tgt.d_tidx.reset();
    if (!(c->tgt.filter_ok && c->tune.nn_sort && c->tgt.nt >= 2)) return OA_OK;
    const double *lo = c->bb_lo, *hi = c->bb_hi;
    const int ad = c->fax[2];
    int su = 0;
    for (int a = 1; a < 3; ++a) if (hi[a] - lo[a] > hi[su] - lo[su]) su = a;
    const int sd = ad != su ? ad : (su + 1) % 3;                   // (all extents equal: any other axis)
    c->sax[0] = su; c->sax[2] = sd; c->sax[1] = 3 - su - sd;
    const double ext = hi[su] - lo[su];
    const int blocks = (c->tgt.n_groups_pad + 255) / 256;
    DevTmp<unsigned> k_in;
    DevTmp<int> v_out;
    HIPCHK(k_in.alloc((size_t)c->tgt.nt)); HIPCHK(v_out.alloc((size_t)c->tgt.nt));
    hipLaunchKernelGGL(oa::k_sort_keys_axis, dim3((c->tgt.nt + 255) / 256), dim3(256), 0, c->stream, (const float *)c->tgt.d_tgt_xyz, c->tgt.nt, su, lo[su],
                       ext > 0.0 ? 1073741823.0 / ext : 0.0, k_in.p);
    HIPCHK(hipGetLastError());
    { const int rcs = sort_order_bits(c, k_in.p, v_out.p, (size_t)c->tgt.nt, 30); if (rcs) return rcs; }
    if (c->tune.nn_vchunk) {                                           // every block of the u order by v, its first vertex kept (k_sort_blocks_v)
        hipLaunchKernelGGL(oa::k_sort_blocks_v, dim3((unsigned)((c->tgt.nt + oa::SORTED_VBLOCK - 1) / oa::SORTED_VBLOCK)), dim3(oa::SORTED_VBLOCK), 0,
                           c->stream, (const float *)c->tgt.d_tgt_xyz, c->tgt.nt, c->sax[1], c->tc[c->sax[1]], v_out.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(dev_malloc(&c->tgt.d_tfs, sizeof(float4) * 3 * (size_t)c->tgt.n_groups_pad));
    HIPCHK(dev_malloc(&c->tgt.d_tf3s, sizeof(float4) * 2 * (size_t)c->tgt.n_groups_pad));
    HIPCHK(dev_malloc(&c->tgt.d_tgs, sizeof(float4) * 3 * (size_t)c->tgt.n_groups_pad));
    HIPCHK(dev_malloc(&c->tgt.d_tidx, sizeof(int4) * (size_t)c->tgt.n_groups_pad));
    HIPCHK(dev_malloc(&c->tgt.d_tmw, sizeof(float4) * (size_t)c->tgt.n_groups_pad));
    // (every kind of level 0 gets its images -- tmw and toct: which a search reads follows from its source's R, oa::sorted_level0)
    const int n_images = c->tgt.n_groups_pad / (oa::SORTED_IMAGE_V / 4);   // (n_groups_pad: a multiple of 256, whole images and whole fours of them)
    HIPCHK(dev_malloc(&c->tgt.d_toct, sizeof(float4) * 3 * (size_t)(n_images / 4)));
    // level 0's cap (oa_octgap.hpp: any value >= 0 is valid, it only tunes what the images' bound loses): the mean half-span in u
    // of a block of 256 sorted vertices -- halves of an image further apart than that are the sparse regions'
    {
        const double cap = ext * 128.0 / (double)c->tgt.nt * oa::SORTED_OCT_CAP;
        c->tgt.oct_c = (cap >= 0.0 && cap < 1e18) ? (float)cap : 0.0f;
    }
    hipLaunchKernelGGL(oa::k_pack_sorted, dim3((unsigned)blocks), dim3(256), 0, c->stream, (const float *)c->tgt.d_tgt_xyz, c->tgt.nt, c->tgt.n_groups_pad,
                       (const int *)v_out.p, c->tc[0], c->tc[1], c->tc[2], c->sax[0], c->sax[1], c->sax[2], c->tgt.d_tfs, c->tgt.d_tf3s, c->tgt.d_tgs, c->tgt.d_tidx, c->tgt.d_tmw);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(oa::k_group_images, dim3((unsigned)((n_images + 255) / 256)), dim3(256), 0, c->stream, (const float4 *)c->tgt.d_tfs,
                       (const int4 *)c->tgt.d_tidx, n_images, c->tgt.oct_c, c->tgt.d_toct);   // (from what k_pack_sorted has written)
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));                      // (the temporaries are released on return)
    return OA_OK;
}

int build_filter(oa_ctx *c, bool vertex_target)
{
    c->tgt.filter_ok = false;
    const int nb = 256;
    std::vector<float> bb(6 * nb);
    { int rcb = bbox_partials(c, c->tgt.d_tgt_xyz, c->tgt.nt, nb, bb.data()); if (rcb) return rcb; }
    float lof[3], hif[3];
    bool finite = !fold_bbox(bb.data(), nb, lof, hif);
    const double lo[3] = { lof[0], lof[1], lof[2] }, hi[3] = { hif[0], hif[1], hif[2] };
    for (int a = 0; a < 3; ++a) if (!(lo[a] <= hi[a]) || !(fabs(lo[a]) < 1e18) || !(fabs(hi[a]) < 1e18)) finite = false;
    if (!finite) return OA_OK;                                   // exact kernel only
    for (int a = 0; a < 3; ++a) { c->tc[a] = (float)(0.5 * (lo[a] + hi[a])); c->bb_lo[a] = lo[a]; c->bb_hi[a] = hi[a]; }
    // the first-level score drops the axis along which the cloud is thinnest (fewest vertices share a projection)
    int ad = 0;
    for (int a = 1; a < 3; ++a) if (hi[a] - lo[a] < hi[ad] - lo[ad]) ad = a;
    c->fax[2] = ad; c->fax[0] = (ad + 1) % 3; c->fax[1] = (ad + 2) % 3;
    if (c->fax[0] > c->fax[1]) std::swap(c->fax[0], c->fax[1]);
    const int blocks = (c->tgt.n_groups_pad + 255) / 256;
    DevTmp<double> d_mx;
#if defined(OA_EXPERIMENTS)        // the images in the caller's order are k_nn_search_filtered's (OA_NN_SORT=0); the launch below still finds qmax
    HIPCHK(dev_malloc(&c->tgt.d_tf, sizeof(float4) * 3 * (size_t)c->tgt.n_groups_pad));
    HIPCHK(dev_malloc(&c->tgt.d_tf3, sizeof(float4) * 2 * (size_t)c->tgt.n_groups_pad));
#endif
    std::vector<double> mx((size_t)blocks);
    {
        // the workgroups' maxima straight into mapped host memory when they fit (result_buffer), else through a device buffer
        void *dv; const void *hv;
        { int rcv = result_buffer(c, sizeof(double) * (size_t)blocks, &dv, &hv); if (rcv) return rcv; }
        if (!dv) HIPCHK(d_mx.alloc((size_t)blocks));
        hipLaunchKernelGGL(oa::k_pack_filter, dim3(blocks), dim3(256), 0, c->stream, c->tgt.d_tgt_xyz, c->tgt.nt, c->tgt.n_groups_pad,
                           c->tc[0], c->tc[1], c->tc[2], c->fax[0], c->fax[1], c->fax[2], c->tgt.d_tf, c->tgt.d_tf3, dv ? (double *)dv : d_mx.p);
        HIPCHK(hipGetLastError());
        if (dv) { HIPCHK(hipStreamSynchronize(c->stream)); memcpy(mx.data(), hv, sizeof(double) * (size_t)blocks); }
        else { int rcr = read_small(c, mx.data(), d_mx, sizeof(double) * (size_t)blocks); if (rcr) return rcr; }
    }
    double m = 0.0;
    for (double v : mx) if (v > m) m = v;
    c->qmax = sqrt(m) * (1.0 + 1e-6);
    c->tgt.filter_ok = (c->qmax < 1e18);
    c->tgt.d_tfs.reset(); c->tgt.d_tf3s.reset(); c->tgt.d_tgs.reset(); c->tgt.d_tmw.reset(); c->tgt.d_toct.reset(); c->tgt.oct_c = 0.0f; c->tgt.d_tidx.reset();
    // k_nn_search_sorted's images are built for the search mode that uses them: a target uploaded for the grid / tree searches
    // (OA_SEARCH_AUTO, the default) does not pay for them; oa_set_search_mode(OA_SEARCH_BRUTE) builds them when it finds none
    // (a mesh's surface searches never launch k_nn_search_sorted: no images, no sort -- ~36 B per vertex)
    if (c->grid_mode == 0 && vertex_target) { const int rcs = build_sorted_images(c); if (rcs) return rcs; }
    c->tgt.d_tfm.reset();
#if defined(OA_EXPERIMENTS)
    if (c->tgt.filter_ok && c->tune.nn_mfma) {                            // experiment: the MFMA image (32 B per target)
        int e = 0;
        if (c->qmax > 0.0) { frexp(c->qmax, &e); }               // qmax = f 2^e, f in [0.5, 1)  ->  qmax 2^-e < 1
        c->mfma_sigma = ldexp(1.0, -e);
        const int n_targets_pad = c->tgt.n_groups_pad * 4;
        HIPCHK(dev_malloc(&c->tgt.d_tfm, sizeof(oa::half8) * 2 * (size_t)n_targets_pad));
        hipLaunchKernelGGL(oa::k_pack_filter_mfma, dim3((unsigned)((n_targets_pad + 255) / 256)), dim3(256), 0, c->stream, c->tgt.d_tgt_xyz,
                           c->tgt.nt, n_targets_pad, c->tc[0], c->tc[1], c->tc[2], c->fax[0], c->fax[1], c->fax[2], c->mfma_sigma, c->tgt.d_tfm);
        HIPCHK(hipGetLastError());
    }
#endif
    return OA_OK;
}

// safe radii per target vertex (k_grid_safe_radius): a seed within its own settles the query without a scan.  One
// launch on the context's stream, no wait: the searches that use the radii are enqueued behind it.
int build_safe_radii(oa_ctx *c)
{
    if (!c->tgt.grid_ok || c->tgt.safe_ok || !c->tgt.d_safe_by_idx || c->tgt.nt < 2) return OA_OK;
    hipLaunchKernelGGL(oa::k_grid_safe_radius, dim3((c->tgt.nt + 255) / 256), dim3(256), 0, c->stream, (const float4 *)c->tgt.d_sorted, c->tgt.nt, c->tgt.gp,
                       (const int *)c->tgt.d_cell_start, c->tgt.d_safe_by_idx);
    HIPCHK(hipGetLastError());
    c->tgt.safe_ok = true;
    return OA_OK;
}

// uniform grid over the target for k_nn_search_grid (needs the finite bbox build_filter found)
int build_grid(oa_ctx *c)
{
    c->tgt.grid_ok = false;
    c->tgt.d_cell_start.reset(); c->tgt.d_sorted.reset(); c->tgt.d_safe_by_idx.reset();
    c->tgt.safe_ok = false;
    if (!c->tgt.filter_ok || c->grid_mode == 0 || c->tgt.nt < 2) return OA_OK;
    if ((long long)c->tgt.nt > oa::GRID_MAX_TARGETS) return OA_OK;       // k_nn_search_grid addresses `sorted` through 32-bit byte offsets; the tree takes over
    double ext[3], vol = 1.0, scale = 0.0;
    int nz = 0;
    for (int a = 0; a < 3; ++a) {
        ext[a] = c->bb_hi[a] - c->bb_lo[a];
        if (ext[a] > 0.0) { vol *= ext[a]; ++nz; }
        scale = std::max(scale, std::max(fabs(c->bb_lo[a]), fabs(c->bb_hi[a])));
    }
    const double ppc = c->tune.grid_ppc;                          // target vertices per cell
    double h = nz ? pow(vol * ppc / (double)c->tgt.nt, 1.0 / nz) : 1.0;
    if (!(h > 0.0) || !(h < INFINITY)) return OA_OK;
    const long long max_cells = 1ll << 24;
    static_assert((1ll << 24) <= oa::GRID_MAX_CELLS, "cell_start is addressed through 32-bit byte offsets");
    DevTmp<int2> d_cell_of;                                         // per vertex {cell, rank inside the cell}
    DevTmp<int> d_counts;
    DevTmp<long long> d_off;
    HIPCHK(d_cell_of.alloc((size_t)c->tgt.nt));
    oa::GridParams gp{};
    int n_cells = 0;
    for (int attempt = 0; attempt < 6; ++attempt) {
        long long total = 1;
        for (int a = 0; a < 3; ++a) {
            long long n = ext[a] > 0.0 ? (long long)floor(ext[a] / h) + 1 : 1;
            n = std::max(1ll, std::min(n, 1024ll));
            gp.n[a] = (int)n;
            total *= n;
            gp.lo[a] = c->bb_lo[a]; gp.hi[a] = c->bb_hi[a];
        }
        if (total > max_cells) { h *= 1.3; n_cells = 0; continue; }
        // a clamped axis (1024 cells) needs a cell edge that still covers the extent
        for (int a = 0; a < 3; ++a) if (ext[a] > 0.0 && ext[a] / h >= gp.n[a]) h = std::max(h, ext[a] / (gp.n[a] - 0.5));
        gp.h = h; gp.inv_h = 1.0 / h;
        gp.r_max = c->tune.grid_rmax;
        gp.seeded_start = c->tune.grid_seeded_start ? 1 : 0;
        // (256: 128 was tuned in round 2, when a hand-over was a list entry; surface-like clouds -- C5 -- keep ~1000 queries per
        //  search above 128 once the doubling for a moving pose ends, and every one of them costs the iteration its fast path)
        gp.budget = c->tune.grid_budget;
        gp.budget_moving = (int)(gp.budget * c->tune.grid_budget_moving);
        gp.moving_h = 0.25 * gp.h;
        gp.slack = 1e-10 * scale + 1e-300;
        gp.scale = scale;
        oa::grid_params_finish(gp);
        n_cells = (int)total;
        // [n_cells]: the scan's closing zero; behind it the occupied-cell counts of k_count_nonzero's workgroups when they do not
        // go to mapped host memory (one memset for all of it: an upload is bound by its number of operations)
        const int nz_blocks = std::min(512, (n_cells + 1023) / 1024);
        HIPCHK(d_counts.alloc((size_t)n_cells + 1 + (size_t)nz_blocks));
        HIPCHK(d_off.alloc((size_t)n_cells + 1));
        void *dv; const void *hv;
        { int rcv = result_buffer(c, sizeof(int) * (size_t)nz_blocks, &dv, &hv); if (rcv) return rcv; }
        int *d_nz = dv ? (int *)dv : d_counts.p + n_cells + 1;
        HIPCHK(hipMemsetAsync(d_counts, 0, sizeof(int) * ((size_t)n_cells + 1), c->stream));
        hipLaunchKernelGGL(oa::k_grid_count, dim3((c->tgt.nt + 255) / 256), dim3(256), 0, c->stream, c->tgt.d_tgt_xyz, c->tgt.nt, gp, d_cell_of.p, d_counts.p);
        hipLaunchKernelGGL(oa::k_count_nonzero, dim3((unsigned)nz_blocks), dim3(1024), 0, c->stream, d_counts.p, n_cells, d_nz);
        HIPCHK(hipGetLastError());
        std::vector<int> nz((size_t)nz_blocks);
        if (dv) { HIPCHK(hipStreamSynchronize(c->stream)); memcpy(nz.data(), hv, sizeof(int) * (size_t)nz_blocks); }
        else { int rcr = read_small(c, nz.data(), d_nz, sizeof(int) * (size_t)nz_blocks); if (rcr) return rcr; }
        long long occupied = 0;
        for (int v : nz) occupied += v;
        const double avg = occupied > 0 ? (double)c->tgt.nt / occupied : 0.0;
        // surfaces fill few cells: refine until occupied cells hold a handful of vertices each
        if (avg > 6.0 && total * 8 <= max_cells && attempt < 5) { h *= 0.5; continue; }
        break;
    }
    if (n_cells <= 0) return OA_OK;
    HIPCHK(dev_malloc(&c->tgt.d_cell_start, sizeof(int) * (size_t)(n_cells + 1)));
    HIPCHK(dev_malloc(&c->tgt.d_sorted, sizeof(float4) * (size_t)c->tgt.nt));
    DevTmp<char> scan_tmp;                                           // released on return, behind the wait below
    { int rcs = scan_counts(c, d_counts.p, n_cells, d_off.p, scan_tmp); if (rcs) return rcs; }
    hipLaunchKernelGGL(oa::k_grid_starts, dim3((n_cells + 256) / 256), dim3(256), 0, c->stream, d_off.p, n_cells, c->tgt.d_cell_start, (int *)nullptr);
    hipLaunchKernelGGL(oa::k_grid_scatter, dim3((c->tgt.nt + 255) / 256), dim3(256), 0, c->stream, c->tgt.d_tgt_xyz, c->tgt.nt, (const int2 *)d_cell_of.p, (const int *)c->tgt.d_cell_start, c->tgt.d_sorted);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    c->tgt.gp = gp; c->tgt.n_cells = n_cells; c->tgt.grid_ok = true;
    c->tgt.target_iters = 0;
    if (c->tune.grid_safe) HIPCHK(dev_malloc(&c->tgt.d_safe_by_idx, sizeof(float) * (size_t)c->tgt.nt));
    if (c->tune.grid_safe == 2) return build_safe_radii(c);
    return OA_OK;
}

// vertex_index = false: the caller (oa_set_target_mesh) searches triangles; the vertex grid and vertex tree would never
// be used (their build is ~40 % of a mesh upload)
int set_target_common(oa_ctx *c, const float *xyz, int64_t n, int on_device, bool vertex_index)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (n < 0 || n > 0x7FFF0000ll) return fail(OA_E_BAD_ARG, "target vertex count %lld out of range", (long long)n);
    if (n > 0 && !xyz) return fail(OA_E_BAD_ARG, "null target pointer");
    int rc = use_device(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->loop_active = false;                                         // an open oa_iterate sequence ends with the old target
    c->tgt = {};                                                    // every image, index and mask of the old target, and what was counted for it
    c->normals_on = false;
    c->tgt.nt = (int)n;
    c->seeded = false; c->win_seeds = false;
    // {index, safe radius} per slot: only the vertex searches read it (8 bytes per source point)
    if (!vertex_index || !c->tune.grid_safe) c->src.d_wsafe.reset();
    else if (c->src.d_prev && !c->src.d_wsafe) HIPCHK(dev_malloc(&c->src.d_wsafe, sizeof(uint2) * (size_t)c->src.ns_pad));
    if (c->src.d_prev) {   // seeds index the old target
        // (the safe radii beside the winner records belong to the old target's indices too)
        hipLaunchKernelGGL(oa::k_init_slots, dim3((c->src.ns_pad + 255) / 256), dim3(256), 0, c->stream, c->src.d_prev, c->src.d_win, c->src.d_wsafe,
                           (unsigned long long *)nullptr, (int *)nullptr, (int *)nullptr, c->src.ns_pad);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (n == 0) return OA_OK;
    HIPCHK(dev_malloc(&c->tgt.d_tgt_xyz, sizeof(float) * 3 * (size_t)n));
    {
        // a device pointer may live on another GPU of the process (multi-device contexts replicate the target)
        const int src_dev = on_device ? pointer_device(xyz) : -1;
        if (on_device && src_dev >= 0 && src_dev != c->device)
            HIPCHK(hipMemcpyPeerAsync(c->tgt.d_tgt_xyz, c->device, xyz, src_dev, sizeof(float) * 3 * (size_t)n, c->stream));
        else
            HIPCHK(hipMemcpyAsync(c->tgt.d_tgt_xyz, xyz, sizeof(float) * 3 * (size_t)n,
                                  on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    }
    const long long groups = (n + 3) / 4;
    const long long tiles = (groups + oa::TILE_GROUPS - 1) / oa::TILE_GROUPS;
    c->tgt.n_groups_pad = (int)(tiles * oa::TILE_GROUPS);
    HIPCHK(dev_malloc(&c->tgt.d_tg, sizeof(float4) * 3 * (size_t)c->tgt.n_groups_pad));
    hipLaunchKernelGGL(oa::k_pack_target, dim3((c->tgt.n_groups_pad + 255) / 256), dim3(256), 0, c->stream, c->tgt.d_tgt_xyz,
                       c->tgt.nt, c->tgt.n_groups_pad, c->tgt.d_tg);
    HIPCHK(hipGetLastError());
    int rcf = build_filter(c, vertex_index);                                      // (waits for the stream when it reads the bounding box: the copy above is done by then)
    if (rcf) return rcf;
    if (vertex_index) {
        if ((rcf = build_grid(c))) return rcf;
        if ((rcf = build_bvh(c, false))) return rcf;
    }
    plan_geometry(c);
    return OA_OK;
}
}  // namespace
OA_EXPORT int oa_set_target(oa_ctx *c, const float *xyz, int64_t n, int on_device)
{
    if (c && !c->subs.empty() && c->loop_active) multi_abort(c);            // a new target ends an open oa_iterate sequence
    OA_ROUTE_ALL_PAR(c, oa_set_target(sub, xyz, n, on_device));             // replicated on every device
    return set_target_common(c, xyz, n, on_device, true);
}

namespace {
// offsets[0..n] = exclusive prefix sums of counts[0..n-1] (offsets[n] = total).
// Enqueued, not waited for: `tmp` (the scan's temporary storage) belongs to the caller, who keeps it until the stream has
// been synchronised (the wait in here was a 20-50 us hole in every grid build).
int scan_counts(oa_ctx *c, const int *d_counts, int n, long long *d_off, DevTmp<char> &tmp)
{
    HIPCHK(tmp.alloc(oa::scan_tmp_bytes((size_t)n)));
    HIPCHK(oa::scan_counts_ll((void *)tmp.p, d_counts, (size_t)n, d_off, c->stream));
    return OA_OK;
}

// 64-ary bounding-box tree over the Morton-sorted vertices (tri = false) or triangles (tri = true), oa_bvh.hpp
int build_bvh(oa_ctx *c, bool tri)
{
    bool &ok = tri ? c->tgt.tbvh_ok : c->tgt.bvh_ok;
    DevBuf<float4> &d_box = tri ? c->tgt.d_tbvh_box : c->tgt.d_bvh_box;
    DevBuf<float4> &d_prims = tri ? c->tgt.d_tbvh_prims : c->tgt.d_bvh_prims;
    oa::BvhParams &bp = tri ? c->tgt.tbvh : c->tgt.bvh;
    ok = false;
    d_box.reset(); d_prims.reset();
    const int n = tri ? c->tgt.n_tris : c->tgt.nt;
    if (!c->tgt.filter_ok || c->grid_mode == 0 || n < 1) return OA_OK;
    return build_bvh_arrays(c, tri, c->tgt.d_tgt_xyz, 3, n, c->bb_lo, c->bb_hi, bp, d_box, d_prims, ok);
}

// the tree itself over n primitives: level sizes, Morton order inside the frame [lo, hi], primitive images, boxes.  ok stays
// false (and nothing is allocated) when the tree would need more than BVH_MAX_LEVELS levels.  Vertices: rows of `stride` floats
// at d_xyz (the target: 3; the packed source rows: 4); triangles: c->tgt.d_tri9.
int build_bvh_arrays(oa_ctx *c, bool tri, const float *d_xyz, int stride, int n, const double frame_lo[3], const double frame_hi[3],
                     oa::BvhParams &bp, DevBuf<float4> &d_box, DevBuf<float4> &d_prims, bool &ok)
{
    bp = oa::BvhParams{};
    bp.n_prims = n;
    long long total = 0;
    int level = 0;
    for (long long cnt = ((long long)n + oa::BVH_W - 1) / oa::BVH_W;; cnt = (cnt + oa::BVH_W - 1) / oa::BVH_W) {
        ++level;
        if (level > oa::BVH_MAX_LEVELS) return OA_OK;
        bp.cnt[level] = (int)cnt;
        bp.off[level] = (int)total;
        total += ((cnt + oa::BVH_W - 1) / oa::BVH_W) * oa::BVH_W;
        if (cnt <= oa::BVH_W) break;
    }
    bp.levels = level;
    double scale = 0.0;
    float lo[3], sc[3];
    for (int a = 0; a < 3; ++a) {
        scale = std::max(scale, std::max(fabs(frame_lo[a]), fabs(frame_hi[a])));
        lo[a] = (float)frame_lo[a];
        const double ext = frame_hi[a] - frame_lo[a];
        sc[a] = ext > 0.0 ? (float)(1023.0 / ext) : 0.f;
    }
    bp.scale = scale;
    bp.slack = 1e-10 * scale + 1e-300;
    const int n_pad = bp.cnt[1] * oa::BVH_W;
    DevTmp<unsigned> k_in;
    DevTmp<int> v_out;
    HIPCHK(k_in.alloc((size_t)n)); HIPCHK(v_out.alloc((size_t)n));
    const dim3 blk(256), grd((unsigned)((n + 255) / 256));
    if (tri) hipLaunchKernelGGL(oa::k_bvh_keys<true>, grd, blk, 0, c->stream, d_xyz, stride, (const float4 *)c->tgt.d_tri9,
                                n, lo[0], lo[1], lo[2], sc[0], sc[1], sc[2], k_in.p);
    else hipLaunchKernelGGL(oa::k_bvh_keys<false>, grd, blk, 0, c->stream, d_xyz, stride, (const float4 *)nullptr,
                            n, lo[0], lo[1], lo[2], sc[0], sc[1], sc[2], k_in.p);
    HIPCHK(hipGetLastError());
    { const int rcs = sort_order_bits(c, k_in.p, v_out.p, (size_t)n, 30); if (rcs) return rcs; }
    HIPCHK(dev_malloc(&d_prims, sizeof(float4) * (tri ? 3 : 1) * (size_t)n_pad));
    HIPCHK(dev_malloc(&d_box, sizeof(float4) * 2 * (size_t)total));
    const dim3 grd_pad((unsigned)((n_pad + 255) / 256));
    if (tri) hipLaunchKernelGGL(oa::k_bvh_gather<true>, grd_pad, blk, 0, c->stream, d_xyz, stride, (const float4 *)c->tgt.d_tri9,
                                (const int *)v_out.p, n, n_pad, d_prims);
    else hipLaunchKernelGGL(oa::k_bvh_gather<false>, grd_pad, blk, 0, c->stream, d_xyz, stride, (const float4 *)nullptr,
                            (const int *)v_out.p, n, n_pad, d_prims);
    HIPCHK(hipGetLastError());
    const dim3 grd1((unsigned)((bp.cnt[1] + 3) / 4));               // one wave per box
    if (tri) hipLaunchKernelGGL(oa::k_bvh_leaf_boxes<true>, grd1, blk, 0, c->stream, (const float4 *)d_prims, n_pad, bp.cnt[1], d_box + 2ll * bp.off[1]);
    else hipLaunchKernelGGL(oa::k_bvh_leaf_boxes<false>, grd1, blk, 0, c->stream, (const float4 *)d_prims, n_pad, bp.cnt[1], d_box + 2ll * bp.off[1]);
    HIPCHK(hipGetLastError());
    for (int l = 2; l <= bp.levels; ++l) {
        hipLaunchKernelGGL(oa::k_bvh_upper_boxes, dim3((unsigned)((bp.cnt[l] + 3) / 4)), blk, 0, c->stream,
                           (const float4 *)(d_box + 2ll * bp.off[l - 1]), bp.cnt[l - 1], bp.cnt[l], d_box + 2ll * bp.off[l]);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    ok = true;
    return OA_OK;
}

// Spatial (Morton) order of the source slots: the points a wave owns are neighbours in space, so the grid search's
// reads are shared instead of scattered and the brute-force filter's slow path fires for fewer waves.  The caller-
// order copy and the permutation stay around for the entry points that return per-point data in vlist order.
// bounding box of a float[3n] array -> Morton scaling (lo, 1023 / extent); ok = false for non-finite coordinates
int morton_frame(oa_ctx *c, const float *d_xyz, long long n_verts, float lo[3], float sc[3], bool &ok)
{
    ok = false;
    const int nb = 256;
    std::vector<float> bb(6 * nb);
    { int rcb = bbox_partials(c, d_xyz, n_verts, nb, bb.data()); if (rcb) return rcb; }
    float hi[3];
    if (fold_bbox(bb.data(), nb, lo, hi)) return OA_OK;             // non-finite coordinates: keep the caller's order
    for (int a = 0; a < 3; ++a) {
        if (!(lo[a] <= hi[a]) || !(fabsf(lo[a]) < 1e18f) || !(fabsf(hi[a]) < 1e18f)) return OA_OK;
        sc[a] = hi[a] > lo[a] ? 1023.0f / (hi[a] - lo[a]) : 0.f;
    }
    ok = true;
    return OA_OK;
}

// order[0 .. n) = the Morton order of the packed points pts[0 .. n): stable by the 30-bit key (10 bits an axis) in morton_frame's
// frame, equal keys in index order.  On the context's stream, no wait.
int morton_order(oa_ctx *c, const float4 *pts, int n, const float lo[3], const float sc[3], int *order)
{
    DevTmp<unsigned> keys;
    HIPCHK(keys.alloc((size_t)n));
    hipLaunchKernelGGL(oa::k_morton_keys, dim3((n + 255) / 256), dim3(256), 0, c->stream, pts, n, lo[0], lo[1], lo[2], sc[0], sc[1], sc[2], keys.p);
    HIPCHK(hipGetLastError());
    return sort_order_bits(c, keys.p, order, (size_t)n, 30);
}

// The whole selection of n points packed in selection order (pts, sel: k_pack_source's images) and its Morton order: order[j] =
// the selection position of the j-th point.  ok = false and nothing allocated for non-finite coordinates.  No wait behind the sort.
int selection_morton_order(oa_ctx *c, const float *d_xyz, long long n_verts, const long long *d_vlist, long long step, int n,
                           DevTmp<float4> &pts, DevTmp<int> &sel, DevTmp<int> &order, bool &ok)
{
    float lo[3], sc[3];
    const int rc = morton_frame(c, d_xyz, n_verts, lo, sc, ok);   // (synchronises the stream)
    if (rc || !ok) return rc;
    HIPCHK(pts.alloc((size_t)n)); HIPCHK(sel.alloc((size_t)n)); HIPCHK(order.alloc((size_t)n));
    hipLaunchKernelGGL(oa::k_pack_source, dim3((n + 255) / 256), dim3(256), 0, c->stream, d_xyz, d_vlist, step, 0ll, (const int *)nullptr, n, n, pts.p, sel.p);
    HIPCHK(hipGetLastError());
    return morton_order(c, pts.p, n, lo, sc, order.p);
}

// Are the shards of a selection ranges of its Morton order (compact regions of space), or of the caller's order?
bool spatial_sharding(const oa_ctx *c, long long n_sel, int shards)
{
    return shards > 1 && n_sel < oa::SORT_MAX_N && c->tune.sort_source && c->tune.shard_spatial;
}

// Positions (in the selection) of the points shard [begin, begin + count) of the Morton-ordered selection holds, in
// ascending order -> members (device).  Left empty (caller falls back to contiguous ranges) for non-finite input.
int spatial_shard_members(oa_ctx *c, const float *d_xyz, long long n_verts, const long long *d_vlist, long long step,
                          long long n_sel, long long begin, int count, DevTmp<int> &members)
{
    bool ok = false;
    DevTmp<float4> all4;
    DevTmp<int> all_sel, order;
    const int rc = selection_morton_order(c, d_xyz, n_verts, d_vlist, step, (int)n_sel, all4, all_sel, order, ok);
    if (rc || !ok) return rc;
    // this shard's range of the order, back in ascending selection position (= the caller's order inside the shard)
    HIPCHK(members.alloc((size_t)count));
    DevTmp<int> ord2;
    HIPCHK(ord2.alloc((size_t)count));
    { const int rcs = sort_ints(c, order.p + begin, members.p, ord2.p, (size_t)count, bits_for(n_sel)); if (rcs) return rcs; }
    HIPCHK(hipStreamSynchronize(c->stream));                      // temporaries are released on return
    return OA_OK;
}

int sort_source_slots(oa_ctx *c, const float *d_xyz, long long n_verts)
{
    float lo[3], sc[3];
    bool ok = false;
    int rcf = morton_frame(c, d_xyz, n_verts, lo, sc, ok);
    if (rcf || !ok) return rcf;
    HIPCHK(dev_malloc(&c->src.d_perm, sizeof(int) * (size_t)c->src.ns));
    { const int rcs = morton_order(c, (const float4 *)c->src.d_src4, c->src.ns, lo, sc, c->src.d_perm); if (rcs) return rcs; }
    // d_src4 / d_sel become the sorted images: the packed buffers change names (they ARE the caller-order copy now) and
    // k_apply_perm fills new ones -- every slot up to ns_pad -- instead of two device-to-device copies in front of it
    // (both new buffers first, the context's pointers only when both exist: a failed allocation leaves the unsorted source in
    //  place -- d_perm without sorted images would send later launches through null pointers)
    DevTmp<float4> src_sorted;
    DevTmp<int> sel_sorted;
    {
        const hipError_t e1 = dev_malloc(&src_sorted, sizeof(float4) * (size_t)c->src.ns_pad);
        const hipError_t e2 = e1 == hipSuccess ? dev_malloc(&sel_sorted, sizeof(int) * (size_t)c->src.ns_pad) : e1;
        if (e2 != hipSuccess) { c->src.d_perm.reset(); return fail(OA_E_HIP, "sort_source_slots: %s", hipGetErrorString(e2)); }
    }
    c->src.d_src4o = std::move(c->src.d_src4); c->src.d_src4 = std::move(src_sorted);
    DevTmp<int> selo = std::move(c->src.d_sel); c->src.d_sel = std::move(sel_sorted);
    hipLaunchKernelGGL(oa::k_apply_perm, dim3((c->src.ns_pad + 255) / 256), dim3(256), 0, c->stream, (const float4 *)c->src.d_src4o,
                       (const int *)selo.p, (const int *)c->src.d_perm, c->src.ns, c->src.ns_pad, c->src.d_src4, c->src.d_sel);
    const hipError_t el = hipGetLastError();
    selo.reset();                                                // (stream ordered: behind the launch above; freed on every path)
    if (el != hipSuccess) return fail(OA_E_HIP, "k_apply_perm: %s", hipGetErrorString(el));
    HIPCHK(hipStreamSynchronize(c->stream));
    return OA_OK;
}

// uniform grid over the triangles' bounding boxes
// diag_sum_known: the sum of the triangles' bounding-box diagonals when the caller has it already (oa_set_target_mesh reads
// it back together with its index check: one host round trip instead of two)
int build_tri_grid(oa_ctx *c, const double *diag_sum_known)
{
    c->tgt.tri_grid_ok = false;
    c->tgt.tri_ring_ok = false; c->tgt.tri_iters = 0;
    c->tgt.tri_fine_ok = false;
    c->tgt.d_tcell_start.reset(); c->tgt.d_tcell_rec.reset(); c->tgt.d_tri_ring.reset();
    c->tgt.d_tfine_table.reset(); c->tgt.d_tfine_rec.reset();
    if (!c->tgt.filter_ok || c->grid_mode == 0 || c->tgt.n_tris < 64) return OA_OK;
    if ((long long)c->tgt.n_tris > (long long)oa::TRI_REC_INDEX_MASK || (long long)c->tgt.n_tris > (long long)oa::TRI_POOL_MAX_TRIS) return OA_OK;     // (28-bit indices in the records, 26 in the pool entries: the tree takes such meshes)
    double diag_sum = 0.0;
    if (diag_sum_known) diag_sum = *diag_sum_known;
    else {
        constexpr size_t SLOT_WORDS = (size_t)oa::TOTAL_SLOTS * oa::TOTAL_STRIDE;
        DevTmp<double> d_sum;
        HIPCHK(d_sum.alloc(SLOT_WORDS));
        HIPCHK(hipMemsetAsync(d_sum, 0, sizeof(double) * SLOT_WORDS, c->stream));
        hipLaunchKernelGGL(oa::k_tri_diag_sum, dim3((c->tgt.n_tris + 255) / 256), dim3(256), 0, c->stream, c->tgt.d_tri9, c->tgt.n_tris, d_sum.p);
        HIPCHK(hipGetLastError());
        double slots[SLOT_WORDS];
        { int rcr = read_small(c, slots, d_sum, sizeof(slots)); if (rcr) return rcr; }
        for (int k = 0; k < oa::TOTAL_SLOTS; ++k) diag_sum += slots[(size_t)k * oa::TOTAL_STRIDE];
    }
    double ext[3], scale = 0.0, max_ext = 0.0;
    for (int a = 0; a < 3; ++a) {
        ext[a] = c->bb_hi[a] - c->bb_lo[a];
        max_ext = std::max(max_ext, ext[a]);
        scale = std::max(scale, std::max(fabs(c->bb_lo[a]), fabs(c->bb_hi[a])));
    }
    c->tgt.tri_mean_diag = diag_sum / (double)c->tgt.n_tris;
    double h = c->tune.tri_cell * diag_sum / (double)c->tgt.n_tris;            // mean triangle bbox diagonals per cell edge (1.5 until the scan
                                                                                 // became VALU-bound at the end of round 3: fewer records per cell now pay)
    if (!(h > 0.0) || !(h < INFINITY)) h = max_ext > 0.0 ? max_ext / 64.0 : 1.0;
    h = std::max(h, max_ext / 1023.0);
    const long long max_cells = 1ll << c->tune.tri_max_cells_log2;
    DevTmp<int> d_counts;
    DevTmp<long long> d_off;
    oa::GridParams gp{};
    int n_cells = 0;
    unsigned long long entries = 0;
    for (int attempt = 0; attempt < 8; ++attempt) {
        long long total = 1;
        for (int a = 0; a < 3; ++a) {
            long long n = ext[a] > 0.0 ? (long long)floor(ext[a] / h) + 1 : 1;
            n = std::max(1ll, std::min(n, 1024ll));
            gp.n[a] = (int)n;
            total *= n;
            gp.lo[a] = c->bb_lo[a]; gp.hi[a] = c->bb_hi[a];
        }
        if (total > max_cells) { h *= 1.3; n_cells = 0; continue; }
        gp.h = h; gp.inv_h = 1.0 / h;
        gp.r_max = c->tune.grid_rmax;
        gp.seeded_start = c->tune.tri_seeded_start ? 1 : 0;
        gp.budget = c->tune.tri_budget;
        gp.budget_moving = std::max(1, std::min((int)(gp.budget * c->tune.tri_budget_moving), 60000));   // (range lengths are 16-bit in the kernel; 2.0 until the scan was shared by the wave)
        gp.scale = scale;
        gp.slack = 1e-10 * scale + 1e-300;
        oa::grid_params_finish(gp);
        gp.eps_plane = (float)(8.0 * 5.9604644775390625e-08 * scale + 1e-37);
        gp.drop_over = c->tune.tri_drop_over;
        gp.moving_h = c->tune.tri_moving_frac * gp.h;
        gp.xcd_chunk = c->tune.tri_xcd_chunk;
        gp.xcd_moving_h = c->tune.tri_xcd_moving_frac * gp.h;
        n_cells = (int)total;
        // (the entry total behind the counts, 8-byte aligned: one memset for both)
        const size_t total_at = ((size_t)n_cells + 2) & ~(size_t)1;
        constexpr size_t SLOT_WORDS = (size_t)oa::TOTAL_SLOTS * oa::TOTAL_STRIDE;       // 8-byte words of the spread total (oa_tri.hpp)
        HIPCHK(d_counts.alloc(total_at + 2 * SLOT_WORDS));
        unsigned long long *d_total = (unsigned long long *)(d_counts.p + total_at);
        HIPCHK(hipMemsetAsync(d_counts, 0, sizeof(int) * (total_at + 2 * SLOT_WORDS), c->stream));
        hipLaunchKernelGGL(oa::k_tri_grid_bin<false>, dim3((c->tgt.n_tris + 255) / 256), dim3(256), 0, c->stream, c->tgt.d_tri9,
                           c->tgt.n_tris, gp, d_counts.p, (const int *)nullptr, (float4 *)nullptr, d_total);
        HIPCHK(hipGetLastError());
        {
            unsigned long long slots[SLOT_WORDS];
            int rcr = read_small(c, slots, d_total, sizeof(slots));
            if (rcr) return rcr;
            entries = 0;
            for (int k = 0; k < oa::TOTAL_SLOTS; ++k) entries += slots[(size_t)k * oa::TOTAL_STRIDE];
        }
        // triangles much larger than a cell explode the lists: coarsen
        if (entries > 32ull * (unsigned long long)c->tgt.n_tris + (1ull << 20) || entries > (unsigned long long)oa::TRI_REC_MAX_ENTRIES) { h *= 2.0; n_cells = 0; continue; }
        break;
    }
    if (n_cells <= 0 || entries == 0) return OA_OK;
    HIPCHK(d_off.alloc((size_t)n_cells + 1));
    HIPCHK(dev_malloc(&c->tgt.d_tcell_start, sizeof(int) * (size_t)(n_cells + 1)));
    HIPCHK(dev_malloc(&c->tgt.d_tcell_rec, sizeof(float4) * 2 * ((size_t)entries + oa::TRI_REC_PAD)));
    HIPCHK(hipMemsetAsync(c->tgt.d_tcell_rec + 2 * (size_t)entries, 0, sizeof(float4) * 2 * oa::TRI_REC_PAD, c->stream));   // triangle 0, see tri_scan_shared
    DevTmp<char> scan_tmp;                                           // released on return, behind the wait below
    { int rcs = scan_counts(c, d_counts.p, n_cells, d_off.p, scan_tmp); if (rcs) return rcs; }
    hipLaunchKernelGGL(oa::k_grid_starts, dim3((n_cells + 256) / 256), dim3(256), 0, c->stream, d_off.p, n_cells, c->tgt.d_tcell_start, d_counts.p);
    hipLaunchKernelGGL(oa::k_tri_grid_bin<true>, dim3((c->tgt.n_tris + 255) / 256), dim3(256), 0, c->stream, c->tgt.d_tri9, c->tgt.n_tris,
                       gp, d_counts.p, (const int *)c->tgt.d_tcell_start, c->tgt.d_tcell_rec, (unsigned long long *)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    c->tgt.tgp = gp;
    c->tgt.n_tri_entries = (long long)entries;
    c->tgt.tri_grid_ok = true;
    if (c->tune.debug)
        fprintf(stderr, "[oa] tri grid: h=%g cells=%dx%dx%d entries=%llu (%.2f per triangle)\n", gp.h, gp.n[0], gp.n[1], gp.n[2],
                entries, (double)entries / c->tgt.n_tris);
    if (c->tune.tri_ring) {
        HIPCHK(dev_malloc(&c->tgt.d_tri_ring, sizeof(int) * (size_t)oa::TRI_RING_STRIDE * (size_t)c->tgt.n_tris));
        if (c->tune.tri_ring == 2) { const int rcr = build_tri_ring(c); if (rcr) return rcr; }
    }
    if (c->tune.tri_fine == 2 || (c->tune.tri_fine == 1 && c->tgt.n_tris >= c->tune.tri_fine_min_tris)) return build_tri_fine(c);
    return OA_OK;
}

// The settled-pose structure (oa_tri_fine.hpp): sparse fine grid, inflated lists of whole triangles.  Built with the mesh (never
// inside a loop: it allocates).  Gives up quietly -- the general search serves everything -- when the lists would explode
// (triangles much larger than a cell after six coarsenings) or take more than OA_TRI_FINE_MAX_MB.
int build_tri_fine(oa_ctx *c)
{
    c->tgt.tri_fine_ok = false;
    c->tgt.d_tfine_table.reset(); c->tgt.d_tfine_rec.reset();
#if !defined(OA_EXPERIMENTS)
    return OA_OK;                                                   // (OA_TRI_FINE is inert in the default library)
#else
    if (!c->tgt.tri_grid_ok || !c->tgt.tbvh_ok || !(c->tgt.tri_mean_diag > 0.0) || !(c->tgt.tri_mean_diag < INFINITY)) return OA_OK;
    oa::FineParams fp{};
    double h = c->tune.tri_fine_cell * c->tgt.tri_mean_diag;
    const double rho_frac = c->tune.tri_fine_rho;
    double ext[3], scale = 0.0, max_ext = 0.0;
    for (int a = 0; a < 3; ++a) {
        ext[a] = c->bb_hi[a] - c->bb_lo[a];
        max_ext = std::max(max_ext, ext[a]);
        scale = std::max(scale, std::max(fabs(c->bb_lo[a]), fabs(c->bb_hi[a])));
    }
    const unsigned long long max_entries = (unsigned long long)(c->tune.tri_fine_max_mb * 1048576.0 / 48.0);
    constexpr size_t SLOT_WORDS = (size_t)oa::TOTAL_SLOTS * oa::TOTAL_STRIDE;
    DevTmp<unsigned long long> d_total;
    HIPCHK(d_total.alloc(SLOT_WORDS));
    unsigned long long entries = 0;
    bool sized = false;
    for (int attempt = 0; attempt < 7 && !sized; ++attempt) {
        fp.rho = rho_frac * h;
        h = std::max(h, (max_ext + 2.0 * fp.rho * (1.0 + 1e-6)) / 1023.0);       // <= 1024 cells per axis: a cell id has 30 bits
        fp.rho = rho_frac * h;
        fp.rho_query = fp.rho * (1.0 - 1e-6);
        fp.h = h; fp.inv_h = 1.0 / h;
        for (int a = 0; a < 3; ++a) {
            fp.lo[a] = c->bb_lo[a] - fp.rho * (1.0 + 1e-6) - 1e-300;
            fp.hi[a] = c->bb_hi[a] + fp.rho * (1.0 + 1e-6) + 1e-300;
            const long long n = (long long)floor((fp.hi[a] - fp.lo[a]) / h) + 1;
            fp.n[a] = (int)std::max(1ll, std::min(n, 1024ll));
        }
        fp.scale = scale;
        fp.slack = 1e-10 * scale + 1e-300;
        HIPCHK(hipMemsetAsync(d_total, 0, sizeof(unsigned long long) * SLOT_WORDS, c->stream));
        hipLaunchKernelGGL(oa::k_tfine_total, dim3((unsigned)((c->tgt.n_tris + 255) / 256)), dim3(256), 0, c->stream, (const float4 *)c->tgt.d_tri9, c->tgt.n_tris, fp, d_total.p);
        HIPCHK(hipGetLastError());
        unsigned long long slots[SLOT_WORDS];
        { int rcr = read_small(c, slots, d_total, sizeof(slots)); if (rcr) return rcr; }
        entries = 0;
        for (int k = 0; k < oa::TOTAL_SLOTS; ++k) entries += slots[(size_t)k * oa::TOTAL_STRIDE];
        if (entries == 0) return OA_OK;
        if (entries > 40ull * (unsigned long long)c->tgt.n_tris + (1ull << 16) || entries > max_entries || entries >= (1ull << 31)) { h *= 1.5; continue; }
        sized = true;
    }
    if (!sized) return OA_OK;
    fp.cap = c->tune.tri_fine_cap;
    fp.gate = c->tune.tri_fine_gate * fp.rho;
    // the table: a power of two of slots, at most a third full for ordinary meshes (7-10 entries per occupied cell); a mesh whose
    // cells hold one entry each overflows the probe limit instead -- then four times the slots, twice
    unsigned long long want = std::max(1024ull, entries / 3ull);
    for (int attempt = 0; attempt < 3; ++attempt, want *= 4ull) {
        int log2 = 10;
        while ((1ull << log2) < want && log2 < 30) ++log2;
        const size_t n_slots = (size_t)1 << log2;
        fp.slots_mask = (unsigned)(n_slots - 1);
        fp.hash_shift = 32 - log2;
        DevTmp<int> d_counts;                                        // [n_slots] counts, then the overflow flag
        DevTmp<long long> d_off;
        DevTmp<char> scan_tmp;
        HIPCHK(dev_malloc(&c->tgt.d_tfine_table, sizeof(uint4) * n_slots));
        HIPCHK(dev_malloc(&c->tgt.d_tfine_rec, sizeof(float4) * 3 * (size_t)entries));
        HIPCHK(d_counts.alloc(n_slots + 2));
        HIPCHK(d_off.alloc(n_slots + 1));
        HIPCHK(hipMemsetAsync(c->tgt.d_tfine_table, 0xFF, sizeof(uint4) * n_slots, c->stream));
        HIPCHK(hipMemsetAsync(d_counts, 0, sizeof(int) * (n_slots + 2), c->stream));
        const dim3 tb((unsigned)((c->tgt.n_tris + 255) / 256));
        hipLaunchKernelGGL(oa::k_tfine_count, tb, dim3(256), 0, c->stream, (const float4 *)c->tgt.d_tri9, c->tgt.n_tris, fp, c->tgt.d_tfine_table, d_counts.p, d_counts.p + n_slots + 1);
        HIPCHK(hipGetLastError());
        { int rcs = scan_counts(c, d_counts.p, (int)n_slots, d_off.p, scan_tmp); if (rcs) return rcs; }
        hipLaunchKernelGGL(oa::k_tfine_fill, tb, dim3(256), 0, c->stream, (const float4 *)c->tgt.d_tri9, c->tgt.n_tris, fp, c->tgt.d_tfine_table, d_counts.p,
                           (const long long *)d_off.p, c->tgt.d_tfine_rec);
        hipLaunchKernelGGL(oa::k_tfine_finish, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, c->stream, c->tgt.d_tfine_table, (int)n_slots,
                           (const long long *)d_off.p);
        HIPCHK(hipGetLastError());
        int overflow = 0;
        { int rcr = read_small(c, &overflow, d_counts.p + n_slots + 1, sizeof(int)); if (rcr) return rcr; }   // (waits for the stream: the temporaries may go)
        if (!overflow) {
            c->tgt.tfp = fp;
            c->tgt.n_fine_entries = (long long)entries;
            c->tgt.tri_fine_ok = true;
            if (c->tune.debug)
                fprintf(stderr, "[oa] tri fine grid: h=%g (%.2f mean diagonals) rho=%g cells=%dx%dx%d entries=%llu (%.2f per triangle, %.0f MB) table 2^%d slots\n",
                        fp.h, fp.h / c->tgt.tri_mean_diag, fp.rho, fp.n[0], fp.n[1], fp.n[2], entries, (double)entries / c->tgt.n_tris, entries * 48.0 / 1048576.0, log2);
            return OA_OK;
        }
        c->tgt.d_tfine_table.reset(); c->tgt.d_tfine_rec.reset();
    }
    return OA_OK;
#endif
}

// neighbour lists + accept radii (oa_tri_ring.hpp): one launch on the context's stream, no wait.  The accept radii are written
// into d_tri9's spare lane, which k_pack_tris left at 0 = "never".
int build_tri_ring(oa_ctx *c)
{
#if !defined(OA_EXPERIMENTS)
    (void)c;
    return OA_OK;                                                   // (OA_TRI_RING is inert in the default library)
#else
    if (!c->tgt.tri_grid_ok || !c->tgt.d_tri_ring || c->tgt.tri_ring_ok) return OA_OK;
    const double cap = std::max(0.01, std::min(c->tune.tri_ring_cap, 1.0)) * c->tgt.tgp.h;
    const dim3 blocks((unsigned)((c->tgt.n_tris + 255) / 256));
    if (c->tune.grid_stats || c->tune.debug) {
        DevTmp<unsigned long long> d_stats;
        HIPCHK(d_stats.alloc(oa::RING_STAT_N));
        HIPCHK(hipMemsetAsync(d_stats, 0, sizeof(unsigned long long) * oa::RING_STAT_N, c->stream));
        hipLaunchKernelGGL(oa::k_tri_ring_build<true>, blocks, dim3(256), 0, c->stream, c->tgt.d_tri9, c->tgt.n_tris, c->tgt.tgp, (const int *)c->tgt.d_tcell_start,
                           (const float4 *)c->tgt.d_tcell_rec, cap, c->tgt.d_tri_ring, d_stats.p);
        HIPCHK(hipGetLastError());
        unsigned long long h[oa::RING_STAT_N];
        { int rcr = read_small(c, h, d_stats, sizeof(h)); if (rcr) return rcr; }
        const double nt = (double)std::max(1ull, h[oa::RING_STAT_TRIS]);
        fprintf(stderr, "[oa] tri ring: %llu triangles, %.2f%% never accept, %.2f%% at the cap (%.3g); per triangle: %.1f records read, %.1f triangles tested, %.2f neighbours\n",
                h[oa::RING_STAT_TRIS], 100.0 * h[oa::RING_STAT_NEVER] / nt, 100.0 * h[oa::RING_STAT_CAPPED] / nt, cap, h[oa::RING_STAT_RECORDS] / nt,
                h[oa::RING_STAT_TESTS] / nt, h[oa::RING_STAT_NEIGHBOURS] / nt);
    } else {
        hipLaunchKernelGGL(oa::k_tri_ring_build<false>, blocks, dim3(256), 0, c->stream, c->tgt.d_tri9, c->tgt.n_tris, c->tgt.tgp, (const int *)c->tgt.d_tcell_start,
                           (const float4 *)c->tgt.d_tcell_rec, cap, c->tgt.d_tri_ring, (unsigned long long *)nullptr);
        HIPCHK(hipGetLastError());
    }
    c->tgt.tri_ring_ok = true;
    return OA_OK;
#endif
}

#if defined(OA_EXPERIMENTS)
// The settled-pose search (oa_tri_fine.hpp) in front: one thread per query, its own cell's list of whole triangles; what it
// does not settle (reach beyond the lists' inflation, crowded cells, no seed) is the list the grid search works through
int launch_tri_settle(oa_ctx *c, int &qcap)
{
    const dim3 sblocks((unsigned)(((long long)c->src.ns * 4 + 255) / 256));     // four lanes per query
    qcap = oa::ulist_cap((int)sblocks.x * 4, 16);                   // 16 queries per wave
    auto launch = [&](auto STATS, unsigned long long *stats) {
        hipLaunchKernelGGL((oa::k_tri_settle<decltype(STATS)::value>), sblocks, dim3(256), 0, c->stream, (const oa::DevState *)c->d_state, (const float4 *)c->src.d_src4, c->src.ns, c->tgt.tfp,
                           (const uint4 *)c->tgt.d_tfine_table, (const float4 *)c->tgt.d_tfine_rec, (const float4 *)c->tgt.d_tri9, (const int *)c->src.d_prev, c->src.d_keys, c->src.d_ulist, qcap,
                           ucount_set(c, c->src.u_slot), ucount_set(c, c->src.u_slot ^ 1), stats);
    };
    if (c->tune.grid_stats) {                                            // OA_GRID_STATS=1: instrumented launch, totals to stderr (one row of 8 for the launch)
        unsigned long long h[8];
        { const int rcs = wave_stats(c, 8, 1, h, [&](unsigned long long *stats) { launch(yes, stats); }); if (rcs) return rcs; }
        fprintf(stderr, "[oa] tri settle: %llu of %d queries settled (%.2f records each); the others: %llu no seed, %llu reach beyond rho, %llu outside the box, "
                        "%llu cell not listed / over the cap\n", h[0], c->src.ns, (double)h[5] / (double)std::max(1ull, h[0]), h[1], h[2], h[3], h[4]);
    } else launch(no, nullptr);
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// With the neighbour lists and seeds: k_tri_accept settles what seed + neighbours settle and lists the rest, the grid search
// works through the list (oa_tri.hpp)
int launch_tri_accept(oa_ctx *c, const int *ring, int &qcap)
{
    qcap = oa::ulist_cap((c->src.ns + 63) / 64, 64);
    hipLaunchKernelGGL(oa::k_tri_accept, dim3((unsigned)((c->src.ns + 255) / 256)), dim3(256), 0, c->stream, (const oa::DevState *)c->d_state,
                       (const float4 *)c->src.d_src4, c->src.ns, (float)c->tgt.tgp.scale * 1.000001f, (const float4 *)c->tgt.d_tri9, (const int *)c->src.d_prev, ring,
                       c->src.d_keys, c->src.d_ulist, qcap, ucount_set(c, c->src.u_slot), ucount_set(c, c->src.u_slot ^ 1));
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// the instrumented plain triangle grid search (one lane per query, workgroups of 256 threads): totals to stderr
template <typename Launch>
int tri_grid_stats(oa_ctx *c, unsigned blocks, Launch &&launch)
{
    unsigned long long h[oa::TRI_STAT_N];
    { const int rcs = wave_stats(c, oa::TRI_STAT_N, (size_t)blocks * 4, h, launch); if (rcs) return rcs; }
    const double nq = (double)std::max(1ull, h[oa::TRI_STAT_QUERIES]), nw = (double)std::max(1ull, h[oa::TRI_STAT_WAVES]);
    fprintf(stderr, "[oa] tri grid stats: queries %llu | per query: rows %.2f entries %.2f (sphere passes %.2f) survivors %.2f evals %.2f | per wave: "
                    "eval trips %.1f max-lane entries %.1f max-lane rows %.1f | ring>=2 %.1f%% ring>=3 %.1f%% unsettled %.1f%% over budget %.1f%%\n",
            h[oa::TRI_STAT_QUERIES], h[oa::TRI_STAT_ROWS] / nq, h[oa::TRI_STAT_ENTRIES] / nq, h[oa::TRI_STAT_SPHERE] / nq, h[oa::TRI_STAT_SURVIVORS] / nq,
            h[oa::TRI_STAT_EVALS] / nq, h[oa::TRI_STAT_WAVE_TRIPS] / nw, h[oa::TRI_STAT_WAVE_MAX_ENTRIES] / nw,
            h[oa::TRI_STAT_WAVE_MAX_ROWS] / nw, 100.0 * h[oa::TRI_STAT_RING2] / nq, 100.0 * h[oa::TRI_STAT_RING3] / nq,
            100.0 * h[oa::TRI_STAT_UNSETTLED] / nq, 100.0 * h[oa::TRI_STAT_OVER] / nq);
    const double ct = (double)std::max(1ull, h[oa::TRI_STAT_CYC_TOTAL]);
    fprintf(stderr, "[oa] tri grid phases: per wave %.0f shader cycles, %.2f loop trips | prologue %.1f%% listing %.1f%% scan %.1f%% flush %.1f%% bookkeeping %.1f%% epilogue %.1f%%\n",
            ct / nw, h[oa::TRI_STAT_LOOP_TRIPS] / nw, 100.0 * h[oa::TRI_STAT_CYC_PROLOGUE] / ct, 100.0 * h[oa::TRI_STAT_CYC_LIST] / ct,
            100.0 * h[oa::TRI_STAT_CYC_SCAN] / ct, 100.0 * h[oa::TRI_STAT_CYC_FLUSH] / ct, 100.0 * h[oa::TRI_STAT_CYC_BOOK] / ct,
            100.0 * (ct - h[oa::TRI_STAT_CYC_PROLOGUE] - h[oa::TRI_STAT_CYC_LIST] - h[oa::TRI_STAT_CYC_SCAN] - h[oa::TRI_STAT_CYC_FLUSH] - h[oa::TRI_STAT_CYC_BOOK]) / ct);
    return OA_OK;
}
#endif

// The triangle grid search; the far queries it hands over go through the triangle tree (a list launch behind it, or -- acc -- the wave that owns them)
int launch_tri_grid(oa_ctx *c, const SearchChoice &s, bool acc)
{
    if (!acc && !c->loop_active) { HIPCHK(hipMemsetAsync(c->src.d_todo_count, 0, TODO_COUNT_INTS * sizeof(int), c->stream)); c->src.u_slot = 0; }
    if (c->loop_active) { const int rcr = tri_ring_lazy(c, true); if (rcr) return rcr; }
    const int *ring = c->tgt.tri_ring_ok ? c->tgt.d_tri_ring : nullptr;
    // a front search (SearchChoice) leaves the list of the queries it did not settle: never for the accumulating form
    bool listed = s.accept_front && ring && !acc && c->src.d_ulist;
    const int *qlist = nullptr, *qcount = nullptr;
    int qcap = 0;
#if defined(OA_EXPERIMENTS)
    const bool settle = s.settle_front && !acc && c->src.d_ulist;
    if (settle || listed) {
        const int rcf = settle ? launch_tri_settle(c, qcap) : launch_tri_accept(c, ring, qcap);
        if (rcf) return rcf;
        qlist = c->src.d_ulist; qcount = ucount_set(c, c->src.u_slot);
        c->src.u_slot ^= 1;
        ring = nullptr;                                             // (the list's queries failed that test already)
        listed = true;
    }
#endif
    if (s.dual) { int rcb = launch_bvh<true>(c, nullptr, nullptr, 1); if (rcb) return rcb; }    // runs when DevState::tree_turn
    const int lanes = s.lanes;
    // k_tri_search_grid<L, STATS, SHARE, ACC, BT>; the accumulating form gets the tree, the pair test and the rows of partials
    auto launch = [&](auto L, auto STATS, auto SHARE, auto ACC, auto BT, unsigned blocks, unsigned long long *stats, const int *kring, int qmin = 0, int qmax = 0x7FFFFFFF) {
        constexpr bool A = decltype(ACC)::value;
        hipLaunchKernelGGL((oa::k_tri_search_grid<decltype(L)::value, decltype(STATS)::value, decltype(SHARE)::value, A, decltype(BT)::value>), dim3(blocks), dim3(decltype(BT)::value), 0, c->stream,
                           c->d_state, c->src.d_src4, c->src.ns, c->tgt.tgp, c->tgt.d_tcell_start, c->tgt.d_tcell_rec, c->tgt.d_tri9, c->src.d_prev, c->src.d_keys, c->src.d_todo_list, c->src.d_todo_count, s.dual ? 0 : -1, stats,
                           A ? c->tgt.tbvh : oa::BvhParams{}, A ? (const float4 *)c->tgt.d_tbvh_box : nullptr, A ? (const float4 *)c->tgt.d_tbvh_prims : nullptr,
                           A ? normal_test(c) : oa::NormalTest{}, A ? c->d_partials : nullptr, kring, qlist, qcount, qmin, qmax, qcap);
    };
    const unsigned gblocks = (unsigned)(((long long)c->src.ns * lanes + 255) / 256);
    if (acc) {
        // the search finishes its own leftovers through the triangle tree and takes the pair test and the sums in its
        // epilogue (PLAN_GRID, fast path): no list launch, no accumulation launch
        dispatch<1, 2, 4>(lanes, [&](auto L) { launch(L, no, yes, yes, int_c<256>{}, gblocks, nullptr, ring); });
        HIPCHK(hipGetLastError());
        return OA_OK;
    }
    // long plain searches: one wave per workgroup (k_tri_search_grid, BT = 64): a slot is free again when ITS wave is through
    const long long wblocks = ((long long)c->src.ns * lanes + 63) / 64;
    if (listed) {
        // the list's length decides the lanes per query, on the device (k_tri_search_grid: qmin / qmax): a 4-lane launch for
        // lists of up to `small` queries, and the shard's own geometry for longer ones
        const int small = std::min(c->src.ns, (c->tgt.n_tris >= 250000 ? 400 : 128) * c->n_cu);
        const bool two = lanes != 4 && c->tune.tri_split_lanes;
        if (two) launch(int_c<4>{}, no, yes, no, int_c<256>{}, (unsigned)(((long long)small * 4 + 255) / 256), nullptr, nullptr, 0, small);
        dispatch<1, 2, 4>(lanes, [&](auto L) { launch(L, no, yes, no, int_c<256>{}, gblocks, nullptr, nullptr, two ? small : 0, 0x7FFFFFFF); });
    }
    else if (c->tune.tri_wave_wgs && !c->tune.grid_stats && c->tune.tri_share && wblocks >= (long long)c->n_cu * 32)
        dispatch<1, 2, 4>(lanes, [&](auto L) { launch(L, no, yes, no, int_c<64>{}, (unsigned)wblocks, nullptr, ring); });
#if defined(OA_EXPERIMENTS)
    else if (lanes == 1 && c->tune.grid_stats) {
        const int rcs = tri_grid_stats(c, gblocks, [&](unsigned long long *stats) {
            if (c->tune.tri_share) launch(int_c<1>{}, yes, yes, no, int_c<256>{}, gblocks, stats, ring);
            else launch(int_c<1>{}, yes, no, no, int_c<256>{}, gblocks, stats, ring);
        });
        if (rcs) return rcs;
    }
    else if (lanes == 1 && !c->tune.tri_share) launch(int_c<1>{}, no, no, no, int_c<256>{}, gblocks, nullptr, ring);
#endif
    else dispatch<1, 2, 4>(lanes, [&](auto L) { launch(L, no, yes, no, int_c<256>{}, gblocks, nullptr, ring); });
    HIPCHK(hipGetLastError());
    if (c->tune.debug && !listed) {                                     // how many queries the grid handed over (debug only: syncs)
        int n_todo = 0;
        { int rcr = read_small(c, &n_todo, c->src.d_todo_count, sizeof(int)); if (rcr) return rcr; }
        fprintf(stderr, "[oa] tri grid handed %d of %d queries to the tree\n", n_todo, c->src.ns);
    }
    return launch_bvh<true>(c, c->src.d_todo_list, c->src.d_todo_count);   // the far queries: tree search
}

int launch_tri_search(oa_ctx *c, const SearchChoice &s, bool acc)
{
    if (c->tune.debug)
        fprintf(stderr, "[oa] tri search: grid=%d acc=%d ns=%d n_tris=%d state=%p src4=%p tri9=%p prev=%p keys=%p todo=%p/%p cells=%p/%p\n",
                (int)(s.kind == SEARCH_GRID), (int)acc, c->src.ns, c->tgt.n_tris, (void *)c->d_state, (void *)c->src.d_src4, (void *)c->tgt.d_tri9, (void *)c->src.d_prev,
                (void *)c->src.d_keys, (void *)c->src.d_todo_list, (void *)c->src.d_todo_count, (void *)c->tgt.d_tcell_start, (void *)c->tgt.d_tcell_rec);
    if (s.kind == SEARCH_GRID) return launch_tri_grid(c, s, acc);
    hipLaunchKernelGGL(oa::k_tri_search_all, dim3(std::min((c->src.ns + 255) / 256, 65535)), dim3(256), 0, c->stream,
                       c->d_state, c->src.d_src4, c->src.ns, c->tgt.d_tri9, c->tgt.n_tris, c->src.d_prev, c->src.d_keys);
    HIPCHK(hipGetLastError());
    return OA_OK;
}
}  // namespace

OA_EXPORT int oa_set_target_mesh(oa_ctx *c, const float *xyz, int64_t n_verts, int on_device, const int32_t *tris,
                                 int64_t n_tris)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (!c->subs.empty() && c->loop_active) multi_abort(c);
    OA_ROUTE_ALL_PAR(c, oa_set_target_mesh(sub, xyz, n_verts, on_device, tris, n_tris));
    if (n_tris < 1 || !tris) return fail(OA_E_BAD_ARG, "oa_set_target_mesh: no triangles");
    if (n_tris > 0x2AAAAAA0ll) return fail(OA_E_BAD_ARG, "too many triangles");
    int rc = set_target_common(c, xyz, n_verts, on_device, false);  // vertex images + bbox + filter; no vertex grid / tree
    if (rc) return rc;
    if (n_verts < 1) return fail(OA_E_BAD_ARG, "oa_set_target_mesh: no vertices");
    DevBuf<int> &d_tris = c->tgt.d_tris;                                      // kept: the pseudo-normals are built from the indices (set_target_common freed the old ones)
    constexpr size_t SLOT_WORDS = (size_t)oa::TOTAL_SLOTS * oa::TOTAL_STRIDE;
    DevTmp<double> d_chk;                                           // [0]: (as int) corners that index outside the vertices; [1 ...]: the spread sum of the bounding-box diagonals (oa_tri.hpp: TOTAL_SLOTS)
    HIPCHK(dev_malloc(&d_tris, sizeof(int) * 3 * (size_t)n_tris));
    HIPCHK(d_chk.alloc(1 + SLOT_WORDS));
    HIPCHK(hipMemcpyAsync(d_tris, tris, sizeof(int) * 3 * (size_t)n_tris, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(d_chk, 0, (1 + SLOT_WORDS) * sizeof(double), c->stream));
    HIPCHK(dev_malloc(&c->tgt.d_tri9, sizeof(float4) * 3 * (size_t)n_tris));
    hipLaunchKernelGGL(oa::k_pack_tris, dim3((unsigned)((n_tris + 255) / 256)), dim3(256), 0, c->stream, c->tgt.d_tgt_xyz,
                       (int)n_verts, (const int *)d_tris, (int)n_tris, c->tgt.d_tri9, (int *)d_chk.p);
    // the triangle grid's cell size comes from the mean bounding-box diagonal: summed here, so that the index check and the
    // sum come back in ONE host round trip (a bad index leaves a triangle of garbage corners: the sum is not used then)
    hipLaunchKernelGGL(oa::k_tri_diag_sum, dim3((unsigned)((n_tris + 255) / 256)), dim3(256), 0, c->stream, c->tgt.d_tri9, (int)n_tris, d_chk.p + 1);
    HIPCHK(hipGetLastError());
    double chk[1 + SLOT_WORDS];
    { int rcr = read_small(c, chk, d_chk, sizeof(chk)); if (rcr) return rcr; }
    int bad = 0;
    memcpy(&bad, &chk[0], sizeof(int));
    double diag_sum = 0.0;
    for (int k = 0; k < oa::TOTAL_SLOTS; ++k) diag_sum += chk[1 + (size_t)k * oa::TOTAL_STRIDE];
    if (bad) { c->tgt.d_tri9.reset(); c->tgt.d_tris.reset(); return fail(OA_E_BAD_ARG, "oa_set_target_mesh: %d triangle corners index outside 0..%lld", bad, (long long)n_verts - 1); }
    c->tgt.n_tris = (int)n_tris;
    c->tgt.surface = true;
    if ((rc = build_bvh(c, true))) return rc;
    return build_tri_grid(c, &diag_sum);
}

namespace {
// n floats of caller data, readable by c's device on c's stream: host data and pointers that live on ANOTHER GPU are
// copied into `tmp` (a kernel of device i must not dereference device j's memory: nothing enables peer access for
// caller buffers); a pointer on c's own device is used as it is
int stage_floats(oa_ctx *c, const float *src, size_t n, int on_device, DevTmp<float> &tmp, const float *&local)
{
    local = src;
    if (n == 0) return OA_OK;
    if (!on_device) {
        HIPCHK(tmp.alloc(n));
        HIPCHK(hipMemcpyAsync(tmp, src, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
        local = tmp;
        return OA_OK;
    }
    const int dev = pointer_device(src);
    if (dev < 0 || dev == c->device) return OA_OK;
    HIPCHK(tmp.alloc(n));
    HIPCHK(hipMemcpyPeerAsync(tmp, c->device, src, dev, sizeof(float) * n, c->stream));
    local = tmp;
    return OA_OK;
}

// release the old shard and allocate everything a shard of `count` selected points needs (seeds cleared, keys empty)
int source_reset(oa_ctx *c, long long count, long long begin, long long n_verts)
{
    HIPCHK(hipStreamSynchronize(c->stream));
    c->loop_active = false;                                         // an open oa_iterate sequence ends with the old source
    c->src = {};                                                    // the old shard: its points, seeds, tree, verdicts and scratch
    { const int rcc = filters_clear(c); if (rcc) return rcc; }      // ... and the old source's counts and figures
    c->src.shard_begin = begin;
    c->normals_on = false;
    c->src.src_n_verts = n_verts;
    c->src.ns = (int)count;
    // points per thread: 4 for big shards; small shards take 2 or 1 so that the launch still has enough workgroups
    c->src.R = c->tune.nn_r ? c->tune.nn_r : (count >= 65536 ? 4 : (count >= 16384 ? 2 : 1));
    const int chunk = oa::NN_THREADS * c->src.R;
    c->src.ns_pad = (int)(((count + chunk - 1) / chunk) * chunk);
    if (c->src.ns_pad == 0) c->src.ns_pad = chunk;
    HIPCHK(dev_malloc(&c->src.d_src4, sizeof(float4) * (size_t)c->src.ns_pad));
    HIPCHK(dev_malloc(&c->src.d_keys, sizeof(unsigned long long) * (size_t)c->src.ns_pad));
    HIPCHK(dev_malloc(&c->src.d_prev, sizeof(int) * (size_t)c->src.ns_pad));
    HIPCHK(dev_malloc(&c->src.d_win, sizeof(float4) * (size_t)c->src.ns_pad));
    if (c->grid_mode == 0) { const int rcq = ensure_sorted_buffers(c, c->src.ns_pad / chunk); if (rcq) return rcq; }   // (brute force only, never inside a loop: 64 B per slot + the brute-force launch's q_blocks, a few KB)
    if (c->tune.grid_safe && !c->tgt.surface) HIPCHK(dev_malloc(&c->src.d_wsafe, sizeof(uint2) * (size_t)c->src.ns_pad));   // (a vertex target set later allocates it: set_target_common)
    c->seeded = false; c->win_seeds = false;
    HIPCHK(dev_malloc(&c->src.d_sel, sizeof(int) * (size_t)c->src.ns_pad));
    HIPCHK(dev_malloc(&c->src.d_todo_list, sizeof(int) * (size_t)c->src.ns_pad));
    HIPCHK(dev_malloc(&c->src.d_ulist, sizeof(int) * ((size_t)c->src.ns_pad + 64 * (size_t)oa::ULIST_PARTS)));   // (ULIST_PARTS regions, each rounded up to whole waves)
    HIPCHK(dev_malloc(&c->src.d_todo_count, TODO_COUNT_INTS * sizeof(int)));      // {entries of the hand-over list, most handed over by one wave, ...}, the two counter sets of d_ulist
    HIPCHK(hipMemsetAsync(c->src.d_todo_count, 0, TODO_COUNT_INTS * sizeof(int), c->stream));
    // no seeds, empty keys, sel = 0, hand-over counters at zero: one launch
    hipLaunchKernelGGL(oa::k_init_slots, dim3((c->src.ns_pad + 255) / 256), dim3(256), 0, c->stream, c->src.d_prev, c->src.d_win, c->src.d_wsafe, c->src.d_keys, c->src.d_sel,
                       c->src.d_todo_count, c->src.ns_pad);
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// one context takes shard shard_index of shard_count: packs (and, for several shards, first Morton-sorts) the
// selection by itself.  The one-process-per-GPU path, single-device contexts, and the fallback of multi-device ones.
int set_source_single(oa_ctx *c, const float *xyz, int64_t n_verts, int on_device, const int64_t *vlist, int64_t n_vlist,
                      long long step, long long n_sel, int32_t shard_index, int32_t shard_count)
{
    const long long per = (n_sel + shard_count - 1) / shard_count;
    const long long begin = std::min(n_sel, per * shard_index);
    const long long count = std::max(0ll, std::min(per, n_sel - begin));
    if (count > oa::SORT_MAX_N) return fail(OA_E_BAD_ARG, "shard too large");
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = source_reset(c, count, begin, n_verts))) return rc;
    c->src_shards = shard_count;
    if (n_sel > 0) {
        const float *d_xyz = xyz;
        DevTmp<float> tmp_xyz;
        DevTmp<long long> d_vlist;
        if ((rc = stage_floats(c, xyz, 3 * (size_t)n_verts, on_device, tmp_xyz, d_xyz))) return rc;
        if (vlist) {
            HIPCHK(d_vlist.alloc((size_t)n_vlist));
            HIPCHK(hipMemcpyAsync(d_vlist, vlist, sizeof(long long) * (size_t)n_vlist, hipMemcpyHostToDevice, c->stream));
        }
        // pivot = first selected vertex of the WHOLE selection (identical on every shard)
        const long long v0 = vlist ? vlist[0] : 0;
        float p0[3];
        if (on_device) HIPCHK(hipMemcpyAsync(p0, d_xyz + 3 * v0, sizeof p0, hipMemcpyDeviceToHost, c->stream));
        else memcpy(p0, xyz + 3 * v0, sizeof p0);
        // Which points of the selection this shard holds.  One shard: all of them.  Several shards: the
        // shard_index-th of shard_count equal ranges of the selection IN MORTON ORDER (every rank sorts the whole
        // selection and gets the same order), so that a shard is a compact region of space -- the brute-force
        // filter and the grid both work per wave of neighbouring points, and a shard that is a sparse sample of the
        // whole cloud costs 16 % more per pair (1/8 of 1M: 7.3 ms vs 6.3 ms).  Fallback (non-finite coordinates,
        // OA_SHARD_SPATIAL=0): contiguous ranges of the selection in the caller's order.
        DevTmp<int> d_members;
        if (c->src.ns > 0 && spatial_sharding(c, n_sel, shard_count)) {
            int rcm = spatial_shard_members(c, d_xyz, n_verts, (const long long *)d_vlist.p, step, n_sel, begin, c->src.ns, d_members);
            if (rcm) return rcm;
            if (d_members.p) {                                      // kept: per-point outputs of a shard go back to vlist order through it
                HIPCHK(dev_malloc(&c->src.d_members, sizeof(int) * (size_t)c->src.ns));
                HIPCHK(hipMemcpyAsync(c->src.d_members, d_members.p, sizeof(int) * (size_t)c->src.ns, hipMemcpyDeviceToDevice, c->stream));
                if (c->parent) {
                    c->src.h_members.resize((size_t)c->src.ns);
                    HIPCHK(hipMemcpyAsync(c->src.h_members.data(), d_members.p, sizeof(int) * (size_t)c->src.ns, hipMemcpyDeviceToHost, c->stream));
                }
            }
        }
        if (c->src.ns > 0) {
            hipLaunchKernelGGL(oa::k_pack_source, dim3((c->src.ns_pad + 255) / 256), dim3(256), 0, c->stream, d_xyz,
                               (const long long *)d_vlist.p, step, begin, (const int *)d_members.p, c->src.ns, c->src.ns_pad, c->src.d_src4, c->src.d_sel);
            HIPCHK(hipGetLastError());
        } else HIPCHK(hipMemsetAsync(c->src.d_src4, 0, sizeof(float4) * (size_t)c->src.ns_pad, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int k = 0; k < 3; ++k) c->src.pivot[k] = (double)p0[k];
        if (c->src.ns > 1 && c->tune.sort_source) {
            int rcs = sort_source_slots(c, d_xyz, n_verts);
            if (rcs) return rcs;
        }
    } else {
        HIPCHK(hipMemsetAsync(c->src.d_src4, 0, sizeof(float4) * (size_t)c->src.ns_pad, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    plan_geometry(c);
    return OA_OK;
}

// The whole selection packed and Morton-sorted ONCE, on one device of a multi-device context (round 2: every device
// sorted the whole selection to find its range -- at 10M points, 8 sorts of 10M keys).  Slot j of the order holds the
// point at selection position pos[j]; shard g of n is the range [g per, g per + count_g) of it -- exactly the slots the
// per-context path (spatial_shard_members + sort_source_slots) ends up with, in the same order: both order the selection with
// selection_morton_order, and sort_source_slots' morton_order of a shard keeps that order (same frame, same key, ties by position).
struct SelectionOrder {
    DevTmp<float4> pts;
    DevTmp<int> sel, pos;
    float p0[3] = { 0.f, 0.f, 0.f };
    bool ok = false;
};

int build_selection_order(oa_ctx *c, const float *xyz, int64_t n_verts, int on_device, const int64_t *vlist, int64_t n_vlist,
                          long long step, long long n_sel, SelectionOrder &o)
{
    o.ok = false;
    int rc = use_device(c);
    if (rc) return rc;
    const float *d_xyz = xyz;
    DevTmp<float> tmp_xyz;
    DevTmp<long long> d_vlist;
    if ((rc = stage_floats(c, xyz, 3 * (size_t)n_verts, on_device, tmp_xyz, d_xyz))) return rc;
    if (vlist) {
        HIPCHK(d_vlist.alloc((size_t)n_vlist));
        HIPCHK(hipMemcpyAsync(d_vlist, vlist, sizeof(long long) * (size_t)n_vlist, hipMemcpyHostToDevice, c->stream));
    }
    const long long v0 = vlist ? vlist[0] : 0;
    if (on_device) HIPCHK(hipMemcpyAsync(o.p0, d_xyz + 3 * v0, sizeof o.p0, hipMemcpyDeviceToHost, c->stream));
    else memcpy(o.p0, xyz + 3 * v0, sizeof o.p0);
    const int n = (int)n_sel;
    bool finite = false;
    DevTmp<float4> all4;
    DevTmp<int> all_sel;
    if ((rc = selection_morton_order(c, d_xyz, n_verts, (const long long *)d_vlist.p, step, n, all4, all_sel, o.pos, finite))) return rc;
    if (!finite) return OA_OK;                                     // caller falls back to contiguous ranges
    HIPCHK(o.pts.alloc((size_t)n)); HIPCHK(o.sel.alloc((size_t)n));
    hipLaunchKernelGGL(oa::k_apply_perm, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const float4 *)all4.p, (const int *)all_sel.p,
                       (const int *)o.pos.p, n, n, o.pts.p, o.sel.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));                      // temporaries are released on return; other devices read the order next
    o.ok = true;
    return OA_OK;
}

// device c takes the range [begin, begin + count) of the order built on `stage`'s device: three range copies over xGMI
// (24 B per point), then a sort of ITS points' selection positions to get back to the caller's order for per-point outputs
int adopt_shard(oa_ctx *c, const oa_ctx *stage, const SelectionOrder &o, long long begin, long long count, long long n_verts)
{
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = source_reset(c, count, begin, n_verts))) return rc;
    for (int k = 0; k < 3; ++k) c->src.pivot[k] = (double)o.p0[k];
    if (count == 0) {
        HIPCHK(hipMemsetAsync(c->src.d_src4, 0, sizeof(float4) * (size_t)c->src.ns_pad, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        plan_geometry(c);
        return OA_OK;
    }
    const int n = (int)count;
    DevTmp<int> pos, inv;
    HIPCHK(pos.alloc((size_t)n)); HIPCHK(inv.alloc((size_t)n));
    const bool local = stage->device == c->device;
#define OA_RANGE_COPY(dst, src, bytes)                                                                                   \
    HIPCHK(local ? hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToDevice, c->stream)                             \
                 : hipMemcpyPeerAsync((dst), c->device, (src), stage->device, (bytes), c->stream))
    OA_RANGE_COPY(c->src.d_src4, o.pts.p + begin, sizeof(float4) * (size_t)n);
    OA_RANGE_COPY(c->src.d_sel, o.sel.p + begin, sizeof(int) * (size_t)n);
    OA_RANGE_COPY(pos.p, o.pos.p + begin, sizeof(int) * (size_t)n);
#undef OA_RANGE_COPY
    // caller order inside the shard = ascending selection position
    HIPCHK(dev_malloc(&c->src.d_members, sizeof(int) * (size_t)n));
    HIPCHK(dev_malloc(&c->src.d_perm, sizeof(int) * (size_t)n));
    HIPCHK(dev_malloc(&c->src.d_src4o, sizeof(float4) * (size_t)c->src.ns_pad));
    // (inv = the shard's slots in ascending selection position: a stable argsort of pos; d_members = pos in that order)
    { const int rcs = sort_ints(c, pos.p, c->src.d_members, inv.p, (size_t)n, 31); if (rcs) return rcs; }
    hipLaunchKernelGGL(oa::k_finish_shard, dim3((c->src.ns_pad + 255) / 256), dim3(256), 0, c->stream, (const int *)inv.p, n, c->src.ns_pad,
                       c->src.d_src4, c->src.d_sel, c->src.d_src4o, c->src.d_perm);
    HIPCHK(hipGetLastError());
    c->src.h_members.resize((size_t)n);
    HIPCHK(hipMemcpyAsync(c->src.h_members.data(), c->src.d_members, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    plan_geometry(c);
    return OA_OK;
}
}  // namespace

OA_EXPORT int oa_set_source(oa_ctx *c, const float *xyz, int64_t n_verts, int on_device, const int64_t *vlist,
                            int64_t n_vlist, int32_t stride, int32_t shard_index, int32_t shard_count)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (n_verts < 0 || (n_verts > 0 && !xyz)) return fail(OA_E_BAD_ARG, "bad source array");
    if (vlist && n_vlist < 0) return fail(OA_E_BAD_ARG, "negative vlist length");
    if (shard_count < 1 || shard_index < 0 || shard_index >= shard_count)
        return fail(OA_E_BAD_ARG, "bad shard %d of %d", shard_index, shard_count);
    const long long step = stride > 1 ? stride : 1;                 // sample > 1 -> vlist[0::sample] (general.py:274)
    const long long n_all = vlist ? n_vlist : n_verts;
    const long long n_sel = (n_all + step - 1) / step;
    if (vlist)
        for (long long i = 0; i < n_vlist; ++i)
            if (vlist[i] < 0 || vlist[i] >= n_verts)
                return fail(OA_E_BAD_ARG, "vlist[%lld] = %lld outside 0..%lld", i, (long long)vlist[i], (long long)n_verts - 1);
    if (c->subs.empty()) return set_source_single(c, xyz, n_verts, on_device, vlist, n_vlist, step, n_sel, shard_index, shard_count);

    // multi-device: child i keeps shard i of n_dev
    if (shard_count != 1) return fail(OA_E_BAD_ARG, "oa_set_source: a multi-device context shards the source itself (pass shard 0 of 1)");
    if (c->loop_active) multi_abort(c);
    c->loop_active = false;
    const int n_dev = (int)c->subs.size();
    const long long per = (n_sel + n_dev - 1) / n_dev;
    if (n_sel > 1 && spatial_sharding(c, n_sel, n_dev) && c->tune.partition_once) {
        // one Morton sort of the selection on the first device, then every device adopts its range of it
        oa_ctx *stage = c->subs[0];
        SelectionOrder order;
        int rc = build_selection_order(stage, xyz, n_verts, on_device, vlist, n_vlist, step, n_sel, order);
        if (rc) return rc;
        if (order.ok) {
            const SelectionOrder *po = &order;
            return route_all_parallel(c, [=](oa_ctx *sub) -> int {
                const long long begin = std::min(n_sel, per * sub->rank);
                const long long count = std::max(0ll, std::min(per, n_sel - begin));
                return adopt_shard(sub, stage, *po, begin, count, n_verts);
            });
        }
    }
    // fallback (non-finite coordinates, a single device, sorting switched off): every child finds its shard itself
    OA_ROUTE_ALL_PAR(c, set_source_single(sub, xyz, n_verts, on_device, vlist, n_vlist, step, n_sel, sub->rank, n_dev));
    return OA_OK;
}

OA_EXPORT int oa_set_normals(oa_ctx *c, const float *src_normals, int64_t n_verts, const float *tgt_normals, int64_t nt,
                             double max_angle_deg)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (!c->subs.empty() && c->loop_active) multi_abort(c);
    OA_ROUTE_ALL_PAR(c, oa_set_normals(sub, src_normals, n_verts, tgt_normals, nt, max_angle_deg));
    if (c->loop_active) { HIPCHK(hipSetDevice(c->device)); HIPCHK(hipStreamSynchronize(c->stream)); c->loop_active = false; }
    c->normals_on = false;
    if (!src_normals || !(max_angle_deg > 0.0) || !(max_angle_deg < 180.0)) return OA_OK;       // switched off
    if (!c->src.d_src4 || !c->src.d_sel) return fail(OA_E_STATE, "oa_set_normals: call oa_set_source first");
    if (c->tgt.nt <= 0) return fail(OA_E_STATE, "oa_set_normals: call oa_set_target first");
    if (n_verts != c->src.src_n_verts) return fail(OA_E_BAD_ARG, "oa_set_normals: %lld source normals for %lld vertices", (long long)n_verts, c->src.src_n_verts);
    // vertex mode without tgt_normals: the target's own normals (oa_set_target_normals, oa_estimate_target_normals) stay in force
    const bool keep_tgt = !c->tgt.surface && !tgt_normals && c->tgt.d_tgt_n;
    if (!c->tgt.surface && !keep_tgt && (!tgt_normals || nt != c->tgt.nt))
        return fail(OA_E_BAD_ARG, "oa_set_normals: vertex mode needs one normal per target vertex (given here, or set / estimated before)");
    int rc = use_device(c);
    if (rc) return rc;
    DevTmp<float> tmp;
    HIPCHK(tmp.alloc(3 * (size_t)n_verts));
    HIPCHK(hipMemcpyAsync(tmp, src_normals, sizeof(float) * 3 * (size_t)n_verts, hipMemcpyHostToDevice, c->stream));
    if (!keep_tgt) c->tgt.d_tgt_n.reset();
    if (!keep_tgt && !c->tgt.surface) c->tgt.bnd_ok = false;                // (a cloud's boundary mask was built from the old normals)
    HIPCHK(dev_malloc(&c->src.d_src_n, sizeof(float) * 3 * (size_t)std::max(1, c->src.ns)));
    if (c->src.ns > 0)
        hipLaunchKernelGGL(oa::k_gather_rows3, dim3((c->src.ns + 255) / 256), dim3(256), 0, c->stream, (const float *)tmp.p,
                           (const int *)c->src.d_sel, c->src.ns, c->src.d_src_n);
    HIPCHK(hipGetLastError());
    if (!c->tgt.surface && !keep_tgt) {
        HIPCHK(dev_malloc(&c->tgt.d_tgt_n, sizeof(float) * 3 * (size_t)nt));
        HIPCHK(hipMemcpyAsync(c->tgt.d_tgt_n, tgt_normals, sizeof(float) * 3 * (size_t)nt, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->cos_min = cos(max_angle_deg * 3.14159265358979323846 / 180.0);
    c->normals_on = true;
    return OA_OK;
}

namespace {
// A changed setting ends the running sequence: the next oa_iterate starts a new one from the current matrix_world (a
// single-device context fetches it first)
int end_sequence(oa_ctx *c)
{
    if (!c->subs.empty()) { if (c->loop_active) multi_abort(c); }
    else if (c->loop_active) {
        int rc = use_device(c);
        if (rc) return rc;
        if ((rc = fetch_state(c))) return rc;
    }
    c->loop_active = false;
    return OA_OK;
}

// ... and a changed filter setting (`which`, counters = its block if it exists) also clears that filter's counters: the last
// step's figures were the old setting's.  (A multi-device parent keeps the setting itself and refuses the loops: its children
// never see it.)
int filter_setting_changed(oa_ctx *c, unsigned which, const void *counters)
{
    if (!counters) return OA_OK;
    const int rc = use_device(c);
    return rc ? rc : filters_clear(c, which);
}
}  // namespace

OA_EXPORT int oa_set_metric(oa_ctx *c, int metric)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (metric != OA_METRIC_POINT && metric != OA_METRIC_PLANE && metric != OA_METRIC_GICP && metric != OA_METRIC_SYMMETRIC)
        return fail(OA_E_BAD_ARG, "metric %d (use OA_METRIC_POINT / OA_METRIC_PLANE / OA_METRIC_GICP / OA_METRIC_SYMMETRIC)", metric);
    if (metric == c->metric) return OA_OK;
    if (const int rc = end_sequence(c)) return rc;
    c->metric = metric;
    OA_ROUTE_ALL(c, oa_set_metric(sub, metric));
    return OA_OK;
}

OA_EXPORT int oa_set_gicp(oa_ctx *c, double epsilon)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (!(epsilon >= 1e-6 && epsilon <= 1.0)) return fail(OA_E_BAD_ARG, "oa_set_gicp: epsilon must be finite and in [1e-6, 1]");
    if (epsilon == c->gicp_eps) return OA_OK;
    if (const int rc = end_sequence(c)) return rc;
    c->gicp_eps = epsilon;
    OA_ROUTE_ALL(c, oa_set_gicp(sub, epsilon));
    return OA_OK;
}

OA_EXPORT int oa_set_robust(oa_ctx *c, int loss, double scale)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (loss != OA_LOSS_NONE && loss != OA_LOSS_HUBER && loss != OA_LOSS_TUKEY && loss != OA_LOSS_CAUCHY)
        return fail(OA_E_BAD_ARG, "oa_set_robust: loss %d (use OA_LOSS_NONE / OA_LOSS_HUBER / OA_LOSS_TUKEY / OA_LOSS_CAUCHY)", loss);
    if (loss != OA_LOSS_NONE && !(scale > 0.0 && scale < INFINITY))
        return fail(OA_E_BAD_ARG, "oa_set_robust: the scale must be finite and > 0 (world units, like thresh)");
    if (loss == OA_LOSS_NONE) scale = 0.0;
    if (loss == c->loss && scale == c->robust_c) return OA_OK;
    if (const int rc = end_sequence(c)) return rc;
    c->loss = loss;
    c->robust_c = scale;
    c->last_robust_c = 0.0;
    OA_ROUTE_ALL(c, oa_set_robust(sub, loss, scale));
    return OA_OK;
}

OA_EXPORT int oa_set_robust_auto(oa_ctx *c, double quantile, double scale_min)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (!(quantile >= 0.0 && quantile <= 1.0))
        return fail(OA_E_BAD_ARG, "oa_set_robust_auto: the quantile must be in (0, 1], or 0 to switch the estimated scale off");
    if (quantile > 0.0 && !(scale_min > 0.0 && scale_min < INFINITY))
        return fail(OA_E_BAD_ARG, "oa_set_robust_auto: the floor of the scale must be finite and > 0 (world units, like thresh)");
    if (quantile == 0.0) scale_min = 0.0;
    if (quantile == c->robust_p && scale_min == c->robust_cmin) return OA_OK;
    if (const int rc = end_sequence(c)) return rc;
    c->robust_p = quantile;
    c->robust_cmin = scale_min;
    c->last_robust_c = 0.0;
    OA_ROUTE_ALL(c, oa_set_robust_auto(sub, quantile, scale_min));
    return OA_OK;
}

OA_EXPORT int oa_set_reciprocal(oa_ctx *c, int on, double ratio)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (!(ratio >= 1.0 && ratio <= 16.0)) return fail(OA_E_BAD_ARG, "oa_set_reciprocal: the ratio must be in [1, 16] (1: strictly mutual)");
    const bool want = on != 0;
    if (want == c->recip_on && ratio == c->recip_ratio) return OA_OK;
    if (const int rc = end_sequence(c)) return rc;
    c->recip_on = want;
    c->recip_ratio = ratio;
    return filter_setting_changed(c, FILTER_RECIP, c->d_recip_count);
}

OA_EXPORT int oa_set_trim(oa_ctx *c, double fraction, double fraction_min, double lambda)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    const bool est = fraction == OA_TRIM_AUTO;
    if (!(fraction == 0.0 || est || (fraction > 0.0 && fraction <= 1.0)))
        return fail(OA_E_BAD_ARG, "oa_set_trim: the fraction must be 0 (off), in (0, 1], or OA_TRIM_AUTO");
    if (est && !(fraction_min > 0.0 && fraction_min <= 1.0)) return fail(OA_E_BAD_ARG, "oa_set_trim: fraction_min must be in (0, 1] when the share is estimated");
    if (!(lambda >= 0.5 && lambda <= 8.0)) return fail(OA_E_BAD_ARG, "oa_set_trim: lambda must be in [0.5, 8]");
    if (!est) fraction_min = c->trim_min;                           // (ignored: the stored one stays)
    if (fraction == c->trim_fraction && fraction_min == c->trim_min && lambda == c->trim_lambda) return OA_OK;
    if (const int rc = end_sequence(c)) return rc;
    c->trim_fraction = fraction;
    c->trim_min = fraction_min;
    c->trim_lambda = lambda;
    return filter_setting_changed(c, FILTER_TRIM, c->d_trim);
}

namespace {
// (k, angle_deg) of the cloud criterion; nt = the resident cloud's size, or 0 when there is none to hold k against
int check_boundary_params(const char *who, int k, double angle_deg, int nt)
{
    if (k < 3 || k > oa::BND_MAX_K || (nt > 0 && k > nt - 1))
        return fail(OA_E_BAD_ARG, "%s: k = %d outside 3 .. min(%d, target vertices - 1)", who, k, oa::BND_MAX_K);
    if (!(angle_deg > 0.0 && angle_deg < 360.0)) return fail(OA_E_BAD_ARG, "%s: angle_deg = %g outside (0, 360)", who, angle_deg);
    return OA_OK;
}
}  // namespace

OA_EXPORT int oa_set_reject_boundary(oa_ctx *c, int on, int k, double angle_deg)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    // (k is held against the target where the masks are built, ensure_boundary: the setting outlives targets, and switching it
    //  off must work on a cloud of any size)
    int rc = check_boundary_params("oa_set_reject_boundary", k, angle_deg, 0);
    if (rc) return rc;
    const bool want = on != 0;
    if (want == c->bnd_on && k == c->bnd_k && angle_deg == c->bnd_angle) return OA_OK;
    if ((rc = end_sequence(c))) return rc;
    c->bnd_on = want;
    c->bnd_k = k;
    c->bnd_angle = angle_deg;
    return filter_setting_changed(c, FILTER_BND, c->d_bnd_count);
}

OA_EXPORT int oa_set_source_weights(oa_ctx *c, const float *w, int64_t n_verts)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (const int rc = end_sequence(c)) return rc;
    OA_ROUTE_ALL_PAR(c, oa_set_source_weights(sub, w, n_verts));      // every child gathers its own shard
    if (!w) {                                                        // switched off
        if (c->src.d_w) { int rc = use_device(c); if (rc) return rc; HIPCHK(hipStreamSynchronize(c->stream)); c->src.d_w.reset(); }
        return OA_OK;
    }
    if (!c->src.d_src4 || !c->src.d_sel) return fail(OA_E_STATE, "oa_set_source_weights: call oa_set_source first");
    if (n_verts != c->src.src_n_verts) return fail(OA_E_BAD_ARG, "oa_set_source_weights: %lld weights for %lld vertices", (long long)n_verts, c->src.src_n_verts);
    for (int64_t i = 0; i < n_verts; ++i)
        if (!(w[i] >= 0.f && w[i] < INFINITY)) return fail(OA_E_BAD_ARG, "oa_set_source_weights: weight %lld is negative or not finite", (long long)i);
    int rc = use_device(c);
    if (rc) return rc;
    DevTmp<float> tmp;
    HIPCHK(tmp.alloc((size_t)std::max<int64_t>(1, n_verts)));
    HIPCHK(hipMemcpyAsync(tmp, w, sizeof(float) * (size_t)n_verts, hipMemcpyHostToDevice, c->stream));
    if (!c->src.d_w) HIPCHK(dev_malloc(&c->src.d_w, sizeof(float) * (size_t)std::max(1, c->src.ns)));
    if (c->src.ns > 0)
        hipLaunchKernelGGL(oa::k_gather_rows1, dim3((c->src.ns + 255) / 256), dim3(256), 0, c->stream, (const float *)tmp.p,
                           (const int *)c->src.d_sel, c->src.ns, c->src.d_w);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return OA_OK;
}

OA_EXPORT int oa_set_target_normals(oa_ctx *c, const float *tgt_normals, int64_t nt)
{
    if (!c || !tgt_normals) return fail(OA_E_BAD_ARG, "oa_set_target_normals: null argument");
    if (!c->subs.empty() && c->loop_active) multi_abort(c);
    OA_ROUTE_ALL_PAR(c, oa_set_target_normals(sub, tgt_normals, nt));
    if (c->tgt.nt <= 0) return fail(OA_E_STATE, "oa_set_target_normals: call oa_set_target first");
    if (c->tgt.surface) return fail(OA_E_STATE, "oa_set_target_normals: a surface target (oa_set_target_mesh) uses its triangles' geometric normals");
    if (nt != c->tgt.nt) return fail(OA_E_BAD_ARG, "oa_set_target_normals: %lld normals for %d target vertices", (long long)nt, c->tgt.nt);
    int rc = use_device(c);
    if (rc) return rc;
    if (c->loop_active) { HIPCHK(hipStreamSynchronize(c->stream)); c->loop_active = false; }
    if (c->normals_on) HIPCHK(hipStreamSynchronize(c->stream));    // (the array the normal-angle test reads is replaced in place)
    if (!c->tgt.d_tgt_n) HIPCHK(dev_malloc(&c->tgt.d_tgt_n, sizeof(float) * 3 * (size_t)nt));
    c->tgt.bnd_ok = false;                                              // (a boundary mask was built from the old normals)
    HIPCHK(hipMemcpyAsync(c->tgt.d_tgt_n, tgt_normals, sizeof(float) * 3 * (size_t)nt, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return OA_OK;
}

OA_EXPORT int oa_set_source_normals(oa_ctx *c, const float *src_normals, int64_t n_verts)
{
    if (!c || !src_normals) return fail(OA_E_BAD_ARG, "oa_set_source_normals: null argument");
    if (!c->subs.empty() && c->loop_active) multi_abort(c);
    OA_ROUTE_ALL_PAR(c, oa_set_source_normals(sub, src_normals, n_verts));      // every child gathers its own shard
    if (!c->src.d_src4 || !c->src.d_sel) return fail(OA_E_STATE, "oa_set_source_normals: call oa_set_source first");
    if (n_verts != c->src.src_n_verts) return fail(OA_E_BAD_ARG, "oa_set_source_normals: %lld source normals for %lld vertices", (long long)n_verts, c->src.src_n_verts);
    int rc = use_device(c);
    if (rc) return rc;
    if (c->loop_active) { HIPCHK(hipStreamSynchronize(c->stream)); c->loop_active = false; }
    if (c->normals_on) HIPCHK(hipStreamSynchronize(c->stream));    // (the array the normal-angle test reads is replaced in place)
    DevTmp<float> tmp;
    HIPCHK(tmp.alloc(3 * (size_t)std::max<int64_t>(1, n_verts)));
    HIPCHK(hipMemcpyAsync(tmp, src_normals, sizeof(float) * 3 * (size_t)n_verts, hipMemcpyHostToDevice, c->stream));
    if (!c->src.d_src_n) HIPCHK(dev_malloc(&c->src.d_src_n, sizeof(float) * 3 * (size_t)std::max(1, c->src.ns)));
    if (c->src.ns > 0)
        hipLaunchKernelGGL(oa::k_gather_rows3, dim3((c->src.ns + 255) / 256), dim3(256), 0, c->stream, (const float *)tmp.p,
                           (const int *)c->src.d_sel, c->src.ns, c->src.d_src_n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return OA_OK;
}

OA_EXPORT int oa_set_matrices(oa_ctx *c, const float mx_align[16], const float mx_base[16])
{
    if (!c || !mx_align || !mx_base) return fail(OA_E_BAD_ARG, "oa_set_matrices: null argument");
    if (!c->subs.empty()) c->loop_active = false;
    OA_ROUTE_ALL(c, oa_set_matrices(sub, mx_align, mx_base));
    float i1[16], i2[16];
    if (!oa::m4_inverted(mx_align, i1)) return fail(OA_E_SINGULAR, "align matrix_world has no inverse");
    if (!oa::m4_inverted(mx_base, i2)) return fail(OA_E_SINGULAR, "base matrix_world has no inverse");
    memcpy(c->h_state.mx1, mx_align, sizeof i1);
    memcpy(c->h_state.mx2, mx_base, sizeof i1);
    memcpy(c->h_state.imx1, i1, sizeof i1);
    memcpy(c->h_state.imx2, i2, sizeof i2);
    c->have_mats = true;
    c->loop_active = false;
    c->last_todo_wave_max = -1;                                     // a new pose: what the last loop handed over says nothing about the next one
    return OA_OK;
}

OA_EXPORT int oa_reset_seeds(oa_ctx *c)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (!c->subs.empty()) { if (c->loop_active) multi_abort(c); c->loop_active = false; }
    OA_ROUTE_ALL(c, oa_reset_seeds(sub));
    c->seeded = false; c->win_seeds = false;
    c->loop_active = false;
    if (!c->src.d_prev) return OA_OK;
    int rc = use_device(c);
    if (rc) return rc;
    hipLaunchKernelGGL(oa::k_init_slots, dim3((c->src.ns_pad + 255) / 256), dim3(256), 0, c->stream, c->src.d_prev, c->src.d_win, c->src.d_wsafe,
                       (unsigned long long *)nullptr, (int *)nullptr, (int *)nullptr, c->src.ns_pad);
    HIPCHK(hipGetLastError());
    return OA_OK;
}

OA_EXPORT int oa_get_stat(oa_ctx *c, int what, double *value)
{
    if (!c || !value) return fail(OA_E_BAD_ARG, "oa_get_stat: null argument");
    if (what == OA_STAT_CACHE_BYTES) { *value = (double)dev_cache().cached_bytes; return OA_OK; }
    if (what == OA_STAT_ENQUEUED_MIN || what == OA_STAT_ENQUEUED_MAX || what >= OA_STAT_ENQUEUED_CHILD) {
        // iterations the host enqueued for the children in the last oa_run (the agreement of docs/HISTORY.md 4.7: all equal)
        if (c->subs.empty()) { *value = (double)c->iter_enq; return OA_OK; }
        if (what >= OA_STAT_ENQUEUED_CHILD) {
            const size_t i = (size_t)(what - OA_STAT_ENQUEUED_CHILD);
            if (i >= c->subs.size()) return fail(OA_E_BAD_ARG, "oa_get_stat: child %zu of %zu", i, c->subs.size());
            *value = (double)c->subs[i]->enq_iters;
            return OA_OK;
        }
        long long lo = c->subs[0]->enq_iters, hi = lo;
        for (oa_ctx *sub : c->subs) { lo = std::min(lo, sub->enq_iters); hi = std::max(hi, sub->enq_iters); }
        *value = (double)(what == OA_STAT_ENQUEUED_MIN ? lo : hi);
        return OA_OK;
    }
    if (what == OA_STAT_NN_MS_MIN || what == OA_STAT_NN_MS_MAX) {
        if (c->subs.empty()) return fail(OA_E_STATE, "oa_get_stat: per-device search times are a multi-device context's");
        double lo = c->subs[0]->last_nn_ms, hi = lo;
        for (oa_ctx *sub : c->subs) { lo = std::min(lo, sub->last_nn_ms); hi = std::max(hi, sub->last_nn_ms); }
        *value = what == OA_STAT_NN_MS_MIN ? lo : hi;
        return OA_OK;
    }
    if (what == OA_STAT_TRI_RING_ACCEPTS) {
        // the prologue's test of k_tri_search_grid, counted: device state (pose) and seeds as the last search / loop left them
        *value = 0.0;
        if (!c->subs.empty()) {
            for (oa_ctx *sub : c->subs) { double v = 0.0; const int rc = oa_get_stat(sub, what, &v); if (rc) return rc; *value += v; }
            return OA_OK;
        }
        if (!c->tgt.surface || !c->tgt.tri_ring_ok || !c->tgt.d_tri_ring || !c->src.d_prev || !c->d_state || c->src.ns <= 0 || !c->seeded) return OA_OK;
#if defined(OA_EXPERIMENTS)
        int rc = use_device(c);
        if (rc) return rc;
        DevTmp<unsigned long long> d_n;
        HIPCHK(d_n.alloc(16));
        HIPCHK(hipMemsetAsync(d_n, 0, 16 * sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(oa::k_tri_ring_count, dim3((unsigned)((c->src.ns + 255) / 256)), dim3(256), 0, c->stream, (const oa::DevState *)c->d_state,
                           (const float4 *)c->src.d_src4, c->src.ns, c->tgt.tgp.scale, (const float4 *)c->tgt.d_tri9, (const int *)c->src.d_prev, d_n.p,
                           c->tune.debug ? d_n.p : (unsigned long long *)nullptr);
        HIPCHK(hipGetLastError());
        unsigned long long n[16];
        if ((rc = read_small(c, n, d_n, sizeof(n)))) return rc;
        *value = (double)n[0];
        if (c->tune.debug)
            fprintf(stderr, "[oa] tri ring: %llu of %d queries settled by seed + neighbours; the others: %llu no seed, %llu seeds that never accept, %llu not certified, "
                            "distance + margins within 1x / 2x / 4x / 8x of the radius %llu / %llu / %llu / %llu, farther %llu\n",
                    n[0], c->src.ns, n[1], n[2], n[3], n[4], n[5], n[6], n[7], n[8]);
#endif
        return OA_OK;
    }
    if (what == OA_STAT_EXCHANGE_US) {                                  // the slowest device's mean wait for the world's sums (one GPU: 0)
        *value = c->last_exchange_us;
        for (oa_ctx *sub : c->subs) *value = std::max(*value, sub->last_exchange_us);
        return OA_OK;
    }
    if (what == OA_STAT_BRUTE_QUEUE_WGS) { *value = (double)(c->subs.empty() ? c : c->subs[0])->last_queue_wgs; return OA_OK; }
    if (what == OA_STAT_SEARCH_CLOCK_MHZ) {                             // (the host mirror holds the device state of the last oa_run / oa_run_end)
        const oa_ctx *s = c->subs.empty() ? c : c->subs[0];
        const unsigned long long cyc = s->h_state.search_clk[0], ticks = s->h_state.search_clk[1];
        *value = ticks > 0 ? (double)cyc / (double)ticks * s->wall_clock_khz * 1e-3 : 0.0;
        return OA_OK;
    }
    if (what == OA_STAT_RCCL_FALLBACKS) { *value = c->xch && !c->parent ? (double)c->xch->rccl_fallbacks : 0.0; return OA_OK; }
    if (what == OA_STAT_RCCL_RANKS_LAST) { *value = c->xch && !c->parent ? (double)c->xch->rccl_ranks_last : 0.0; return OA_OK; }
    if (what == OA_STAT_WATCHDOG_ABORTS) { *value = c->xch && !c->parent ? (double)c->xch->watchdog_aborts : 0.0; return OA_OK; }
    if (what == OA_STAT_EXCHANGE || what == OA_STAT_RCCL_RANKS || what == OA_STAT_ENQUEUE_US || what == OA_STAT_HOST_THREADS) {
        if (c->subs.empty()) { *value = what == OA_STAT_EXCHANGE ? -1.0 : (what == OA_STAT_HOST_THREADS ? 1.0 : 0.0); return OA_OK; }
        if (what == OA_STAT_HOST_THREADS) { *value = (double)std::max<size_t>(1, c->groups.size()); return OA_OK; }
        if (what == OA_STAT_ENQUEUE_US) {
            double us = 0.0;
            for (oa_ctx *sub : c->subs) if (sub->enq_iters > 0) us = std::max(us, sub->enq_ns / (double)sub->enq_iters * 1e-3);
            *value = us;
            return OA_OK;
        }
        if (!c->loop_active) { const int rcx = exchange_resolve(c); if (rcx) return rcx; }
        if (what == OA_STAT_EXCHANGE) *value = c->xch->mode == OA_EXCHANGE_RCCL ? 1.0 : (c->xch->device_box ? 2.0 : 0.0);
        else *value = (double)exchange_rccl_ranks(c->xch);
        return OA_OK;
    }
    if (what == OA_STAT_RECIPROCAL) { *value = c->recip_on ? 1.0 : 0.0; return OA_OK; }
    if (what == OA_STAT_RECIPROCAL_RATIO) { *value = c->recip_ratio; return OA_OK; }
    if (what == OA_STAT_RECIP_REJECTED || what == OA_STAT_BOUNDARY_REJECTED) {     // word 2 of the filter's counters: the last step's
        const bool recip = what == OA_STAT_RECIP_REJECTED;
        const unsigned *d_count = recip ? c->d_recip_count : c->d_bnd_count;
        *value = 0.0;
        if (!(recip ? c->recip_on : c->bnd_on) || !d_count) return OA_OK;
        int rc = use_device(c);
        if (rc) return rc;
        unsigned n = 0;
        if ((rc = read_small(c, &n, d_count + 2, sizeof n))) return rc;
        *value = (double)n;
        return OA_OK;
    }
    if (what == OA_STAT_REJECT_BOUNDARY) { *value = c->bnd_on ? 1.0 : 0.0; return OA_OK; }
    if (what == OA_STAT_TRIM) { *value = c->trim_fraction; return OA_OK; }
    if (what == OA_STAT_TRIM_CANDIDATES || what == OA_STAT_TRIM_KEPT || what == OA_STAT_TRIM_CUT) {
        *value = 0.0;
        if (!trim_on(c) || !c->d_trim) return OA_OK;
        int rc = use_device(c);
        if (rc) return rc;
        oa::DevTrim t;
        if ((rc = read_small(c, &t, c->d_trim, sizeof t))) return rc;
        *value = what == OA_STAT_TRIM_CANDIDATES ? (double)t.stat_kq : what == OA_STAT_TRIM_KEPT ? (double)t.stat_kept : t.stat_q;
        return OA_OK;
    }
    OA_ROUTE_FIRST(c, oa_get_stat(sub, what, value));
    switch (what) {
    case OA_STAT_GRID_CELLS: *value = c->tgt.grid_ok ? (double)c->tgt.n_cells : 0.0; return OA_OK;
    case OA_STAT_TRI_GRID_CELLS: *value = c->tgt.tri_grid_ok ? (double)c->tgt.tgp.n[0] * c->tgt.tgp.n[1] * c->tgt.tgp.n[2] : 0.0; return OA_OK;
    case OA_STAT_TRI_GRID_ENTRIES: *value = c->tgt.tri_grid_ok ? (double)c->tgt.n_tri_entries : 0.0; return OA_OK;
    case OA_STAT_N_TRIS: *value = (double)c->tgt.n_tris; return OA_OK;
    case OA_STAT_SURFACE: *value = c->tgt.surface ? 1.0 : 0.0; return OA_OK;
    case OA_STAT_BRUTE_KERNEL:
        *value = (double)brute_kernel(c);
        return OA_OK;
    case OA_STAT_FAST_ITERATIONS: *value = (double)c->fast_iters; return OA_OK;
    case OA_STAT_ACC_PATH: *value = (double)c->last_acc_path; return OA_OK;
    case OA_STAT_ACC_ROWS: *value = (double)c->last_acc_rows; return OA_OK;
    case OA_STAT_HANDOVER_ENTRIES: *value = c->h_poll ? (double)c->h_poll[2] : 0.0; return OA_OK;
    case OA_STAT_HANDOVER_WAVE_MAX: *value = c->h_poll ? (double)c->h_poll[3] : 0.0; return OA_OK;
    case OA_STAT_SAFE_RADII: *value = (c->tune.grid_safe && c->tgt.safe_ok) ? 1.0 : 0.0; return OA_OK;
    case OA_STAT_TRI_RING: *value = (c->tune.tri_ring && c->tgt.tri_ring_ok) ? 1.0 : 0.0; return OA_OK;
    case OA_STAT_METRIC: *value = (double)c->metric; return OA_OK;
    case OA_STAT_PLANE_RANK: *value = (double)c->last_plane_rank; return OA_OK;
    case OA_STAT_ROBUST_LOSS: *value = (double)c->loss; return OA_OK;
    case OA_STAT_WEIGHT_SUM: *value = c->last_weight_sum; return OA_OK;
    case OA_STAT_ROBUST_SCALE: *value = c->loss == OA_LOSS_NONE ? 0.0 : (auto_scale(c) ? c->last_robust_c : c->robust_c); return OA_OK;
    case OA_STAT_ROBUST_QUANTILE: *value = c->robust_p; return OA_OK;
    case OA_STAT_TARGET_NORMALS: *value = (!c->tgt.surface && c->tgt.d_tgt_n) ? 1.0 : 0.0; return OA_OK;
    case OA_STAT_TARGET_FEATURES: *value = c->tgt.d_tgt_feat ? 1.0 : 0.0; return OA_OK;
    case OA_STAT_TARGET_BOUNDARY: *value = c->tgt.bnd_ok ? 1.0 : 0.0; return OA_OK;
    case OA_STAT_BOUNDARY_VERTICES: *value = c->tgt.bnd_ok ? (double)c->tgt.bnd_n_vertices : 0.0; return OA_OK;
    case OA_STAT_BOUNDARY_EDGES: *value = c->tgt.bnd_ok ? (double)c->tgt.bnd_n_edges : 0.0; return OA_OK;
    case OA_STAT_MESH_PSEUDONORMALS: *value = (c->tgt.surface && c->tgt.pn_ok) ? 1.0 : 0.0; return OA_OK;
    case OA_STAT_TARGET_CLEANED: *value = (double)c->tgt.cleaned; return OA_OK;
    default: return fail(OA_E_BAD_ARG, "oa_get_stat: unknown key %d", what);
    }
}

OA_EXPORT int oa_get_matrix_world(oa_ctx *c, float mx_align[16])
{
    if (!c || !mx_align) return fail(OA_E_BAD_ARG, "null argument");
    OA_ROUTE_FIRST(c, oa_get_matrix_world(sub, mx_align));           // identical on every device
    if (!c->have_mats) return fail(OA_E_STATE, "matrices not set");
    memcpy(mx_align, c->h_state.mx1, sizeof(float) * 16);
    return OA_OK;
}

OA_EXPORT int64_t oa_num_selected(oa_ctx *c)
{
    if (!c) return 0;
    if (c->subs.empty()) return c->src.ns;
    int64_t n = 0;
    for (oa_ctx *sub : c->subs) n += sub->src.ns;                       // all shards
    return n;
}

OA_EXPORT int oa_get_pivot(oa_ctx *c, double pivot[3])
{
    if (!c || !pivot) return fail(OA_E_BAD_ARG, "null argument");
    OA_ROUTE_FIRST(c, oa_get_pivot(sub, pivot));
    for (int k = 0; k < 3; ++k) pivot[k] = c->src.pivot[k];
    return OA_OK;
}

// search time of every iteration of the last oa_run / oa_run_end, in ms (hipEvent pairs around the brute-force launches, GPU-side
// stamps otherwise): what oa_report::nn_ms_total sums.  A multi-device context answers for its first device.
OA_EXPORT int oa_get_search_ms(oa_ctx *c, int32_t max_n, double *ms)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    OA_ROUTE_FIRST(c, oa_get_search_ms(sub, max_n, ms));
    const int n = std::min((int)c->h_search_ms.size(), (int)std::max(0, max_n));
    for (int i = 0; i < n && ms; ++i) ms[i] = c->h_search_ms[(size_t)i];
    return n;
}

// What the chip's vector ALUs issue RIGHT NOW: burns of dependent-free v_add_f32 / v_min3_f32 chains on every SIMD for ~target_ms, timed
// with hipEvents and with the shader clock / the constant-rate clock read by the same wave at both ends.  bench.py runs it next to
// the headline's timed loop: the brute-force search is bound by VALU issue, the clock under that load is 1.8-2.1 GHz rather
// than the nominal 2.4 and moves from box to box -- with this figure beside it a 50 vs 58 ms launch explains itself.
// out[0] = T lane-ops/s of v_add_f32 (two register sources: the issue rate -- 32 lanes per SIMD and clock), out[1] = shader clock
// (MHz) during that burn, out[2] = duration of both burns (ms), out[3] = T lane-ops/s of v_min3_f32 (the half-rate class the
// search's minimum tree is made of: ~0.55 of out[0])
OA_EXPORT int oa_measure_valu_ceiling(oa_ctx *c, double target_ms, double out[4])
{
    if (!c || !out) return fail(OA_E_BAD_ARG, "oa_measure_valu_ceiling: null argument");
    OA_ROUTE_FIRST(c, oa_measure_valu_ceiling(sub, target_ms, out));
    int rc = use_device(c);
    if (rc) return rc;
    const int wgs_per_cu = 8;                                        // 8 workgroups of 4 waves per CU: 8 waves per SIMD
    const unsigned blocks = (unsigned)(c->n_cu * wgs_per_cu);
    // ~2.7 cycles per wave-instruction and SIMD measured (tools/valu_microbench.hip): iterations for the time asked for
    const double per_iter_s = 8.0 * oa::VALU_BURN_CHAINS * 2.7 / 2.0e9;
    const int iters = ((int)std::max(64.0, std::min(4.0e6, std::max(0.05, std::min(target_ms, 200.0)) * 1e-3 / per_iter_s)) + 7) & ~7;   // (halves are multiples of 4)
    DevTmp<float> d_sink;
    DevTmp<unsigned long long> d_clk;
    HIPCHK(d_sink.alloc((size_t)blocks * 256));
    HIPCHK(d_clk.alloc(4));
    HIPCHK(hipMemsetAsync(d_clk, 0, 4 * sizeof(unsigned long long), c->stream));
    if ((rc = ensure_events(c, 2))) return rc;
    // (a short first launch loads the code object and wakes the clocks; then half the time on each instruction)
    hipLaunchKernelGGL(oa::k_valu_burn<1>, dim3(blocks), dim3(256), 0, c->stream, d_sink.p, 1.0000001f, 1e-9f, std::max(64, (iters / 8) & ~3), d_clk.p);
    HIPCHK(hipEventRecord(c->ev[0], c->stream));
    hipLaunchKernelGGL(oa::k_valu_burn<0>, dim3(blocks), dim3(256), 0, c->stream, d_sink.p, 1.0000001f, 1e-9f, iters / 2, d_clk.p);
    HIPCHK(hipEventRecord(c->ev[1], c->stream));
    HIPCHK(hipEventRecord(c->ev[2], c->stream));
    hipLaunchKernelGGL(oa::k_valu_burn<1>, dim3(blocks), dim3(256), 0, c->stream, d_sink.p, 1.0000001f, 1e-9f, iters / 2, d_clk.p + 2);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev[3], c->stream));
    unsigned long long clk[4];
    if ((rc = read_small(c, clk, d_clk, sizeof(clk)))) return rc;
    float ms_min3 = 0.f, ms_add = 0.f;
    HIPCHK(hipEventElapsedTime(&ms_min3, c->ev[0], c->ev[1]));
    HIPCHK(hipEventElapsedTime(&ms_add, c->ev[2], c->ev[3]));
    const double laneops = (double)blocks * 256.0 * (double)oa::VALU_BURN_CHAINS * (double)(iters / 2);
    out[0] = ms_add > 0.f ? laneops / ((double)ms_add * 1e-3) / 1e12 : 0.0;       // v_add_f32: the issue rate
    out[1] = clk[3] > 0 ? (double)clk[2] / (double)clk[3] * c->wall_clock_khz * 1e-3 : 0.0;
    out[2] = (double)(ms_min3 + ms_add);
    out[3] = ms_min3 > 0.f ? laneops / ((double)ms_min3 * 1e-3) / 1e12 : 0.0;     // v_min3_f32: the half-rate class
    return OA_OK;
}

// ================================================================================================
// correspondence search alone
// ================================================================================================
namespace {
// copies the host mirror (matrices, pivot) to the device with a neutral loop state
int push_state_for_oneshot(oa_ctx *c, double thresh, bool cutoff)
{
    oa_settings st{};
    st.iters = 1; st.use_target = 1; st.with_scale = 0; st.early_exit = 0; st.thresh = thresh; st.target_d = 0.0;
    init_loop_state(c, &st, 1, cutoff);
    HIPCHK(hipStreamSynchronize(c->stream));                    // the staging copy may still be in flight
    int rc = push_state(c);
    if (rc) return rc;
    c->loop_active = false;
    return OA_OK;
}
}  // namespace

OA_EXPORT int oa_nn_search(oa_ctx *c, int64_t *idx, float *d2, double *kernel_ms)
{
    if (c && !c->subs.empty()) {
        // multi-device: every child searches its shard; the answers go back to the caller's (vlist) order through the
        // shard membership each child kept.  kernel_ms = the slowest child (the children run one after the other here:
        // this entry point returns host arrays, it is not the loop).
        if (c->loop_active) multi_abort(c);                          // re-stages every child's device state: the sequence ends
        c->loop_active = false;
        if (kernel_ms) *kernel_ms = 0.0;
        std::vector<int64_t> ic;
        std::vector<float> dc;
        for (oa_ctx *sub : c->subs) {
            const size_t n = (size_t)sub->src.ns;
            if (idx) ic.resize(std::max<size_t>(1, n));
            if (d2) dc.resize(std::max<size_t>(1, n));
            double ms = 0.0;
            int rc = oa_nn_search(sub, idx ? ic.data() : nullptr, d2 ? dc.data() : nullptr, &ms);
            if (rc) return rc;
            if (kernel_ms && ms > *kernel_ms) *kernel_ms = ms;
            for (size_t k = 0; k < n; ++k) {
                const long long g = sub->src.h_members.empty() ? sub->src.shard_begin + (long long)k : (long long)sub->src.h_members[k];
                if (idx) idx[g] = ic[k];
                if (d2) d2[g] = dc[k];
            }
        }
        return OA_OK;
    }
    int rc = check_ready(c);
    if (rc) return rc;
    if ((rc = use_device(c))) return rc;
    if ((rc = ensure_common(c))) return rc;
    if ((rc = ensure_events(c, 1))) return rc;
    if ((rc = push_state_for_oneshot(c, 1.0, false))) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    if (c->src.ns <= 0) return OA_OK;
    DevTmp<long long> d_idx;
    DevTmp<float> d_d2;
    if (idx) HIPCHK(d_idx.alloc((size_t)c->src.ns));
    if (d2) HIPCHK(d_d2.alloc((size_t)c->src.ns));
    HIPCHK(hipEventRecord(c->ev[0], c->stream));
    if ((rc = launch_nn(c, choose_search(c), false))) return rc;
    HIPCHK(hipEventRecord(c->ev[1], c->stream));
    hipLaunchKernelGGL(oa::k_decode_keys, dim3((c->src.ns_pad + 255) / 256), dim3(256), 0, c->stream, c->src.d_keys,
                       c->src.ns_pad, c->src.ns, (const int *)c->src.d_perm, d_idx.p, d_d2.p);
    HIPCHK(hipGetLastError());
    if (idx) HIPCHK(hipMemcpyAsync(idx, d_idx, sizeof(long long) * (size_t)c->src.ns, hipMemcpyDeviceToHost, c->stream));
    if (d2) HIPCHK(hipMemcpyAsync(d2, d_d2, sizeof(float) * (size_t)c->src.ns, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (kernel_ms) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        *kernel_ms = ms;
    }
    return OA_OK;
}

// ================================================================================================
// contract 1: make_pairs
// ================================================================================================
namespace {
// one pass over the pairs, around the pivot c->d_pivot0: the state, the search, the filters (on the point residual: oa_make_pairs
// does not look at the metric), the emitting accumulation (k_pair_accumulate<true>) and its reduce
int make_pairs_pass(oa_ctx *c, double thresh)
{
    int rc;
    if ((rc = push_state_for_oneshot(c, thresh, true))) return rc;
    if ((rc = launch_nn(c, choose_search(c), false))) return rc;
    if ((rc = launch_filters(c, OA_METRIC_POINT, false))) return rc;
    if ((rc = launch_accumulate(c, true, nullptr, nullptr))) return rc;
    return launch_reduce(c, c->d_sums, oa::RowSel{ c->acc_blocks, 0, 0 }, false);
}
}  // namespace

OA_EXPORT int oa_make_pairs(oa_ctx *c, double thresh, int calc_stats, double *A, double *B, int64_t cap, int64_t *K,
                            double dstats[2])
{
    if (c && !c->subs.empty()) {
        if (const int rcf = refuse_filters_multi(c, "oa_make_pairs on a multi-device context")) return rcf;
        // multi-device: every child pairs its shard (its pairs come out in ascending selection position, with that
        // position); the shards are merged back into vlist order on the host.  Statistics: the children's two-pass
        // means and population deviations combine exactly (K-weighted mean; variance = within + between).
        if (!K || cap < 0 || (cap > 0 && (!A || !B))) return fail(OA_E_BAD_ARG, "oa_make_pairs: bad output arguments");
        if (!(thresh > 0.0)) return fail(OA_E_BAD_THRESH, "thresh must be > 0 (the reference's make_pairs returns None)");
        if (c->loop_active) multi_abort(c);                          // re-stages every child's device state: the sequence ends
        c->loop_active = false;
        *K = 0;
        if (dstats) { dstats[0] = NAN; dstats[1] = NAN; }
        const size_t n_dev = c->subs.size();
        std::vector<std::vector<double>> Ac(n_dev), Bc(n_dev);
        std::vector<std::vector<int>> Pc(n_dev);
        std::vector<int64_t> Kc(n_dev, 0);
        std::vector<double> mean(n_dev, 0.0), dev(n_dev, 0.0);
        int64_t total = 0;
        for (size_t r = 0; r < n_dev; ++r) {
            oa_ctx *sub = c->subs[r];
            const int64_t capc = std::max(1, sub->src.ns);
            Ac[r].resize(3 * (size_t)capc); Bc[r].resize(3 * (size_t)capc);
            double st[2] = { NAN, NAN };
            int rc = oa_make_pairs(sub, thresh, calc_stats, Ac[r].data(), Bc[r].data(), capc, &Kc[r], st);
            if (rc) return rc;
            mean[r] = st[0]; dev[r] = st[1];
            Pc[r].resize((size_t)std::max<int64_t>(1, Kc[r]));
            if (Kc[r] > 0) {
                if ((rc = use_device(sub))) return rc;
                HIPCHK(hipMemcpyAsync(Pc[r].data(), sub->src.d_pos, sizeof(int) * (size_t)Kc[r], hipMemcpyDeviceToHost, sub->stream));
                HIPCHK(hipStreamSynchronize(sub->stream));
            }
            total += Kc[r];
        }
        if (total > cap) return fail(OA_E_CAPACITY, "oa_make_pairs: %lld pairs but capacity %lld", (long long)total, (long long)cap);
        std::vector<int64_t> head(n_dev, 0);
        for (int64_t k = 0; k < total; ++k) {                       // n_dev-way merge on the selection position
            size_t best = n_dev;
            for (size_t r = 0; r < n_dev; ++r)
                if (head[r] < Kc[r] && (best == n_dev || Pc[r][(size_t)head[r]] < Pc[best][(size_t)head[best]])) best = r;
            const int64_t h = head[best]++, capc = std::max(1, c->subs[best]->src.ns);
            for (int a = 0; a < 3; ++a) {
                A[(size_t)a * cap + k] = Ac[best][(size_t)a * capc + h];
                B[(size_t)a * cap + k] = Bc[best][(size_t)a * capc + h];
            }
        }
        *K = total;
        if (calc_stats && dstats && total > 0) {
            double m = 0.0;
            for (size_t r = 0; r < n_dev; ++r) if (Kc[r] > 0) m += (double)Kc[r] * mean[r];
            m /= (double)total;
            double var = 0.0;
            for (size_t r = 0; r < n_dev; ++r)
                if (Kc[r] > 0) var += (double)Kc[r] * (dev[r] * dev[r] + (mean[r] - m) * (mean[r] - m));
            dstats[0] = m;
            dstats[1] = sqrt(var / (double)total);
        }
        return OA_OK;
    }
    int rc = check_ready(c);
    if (rc) return rc;
    if (!K || cap < 0 || (cap > 0 && (!A || !B))) return fail(OA_E_BAD_ARG, "oa_make_pairs: bad output arguments");
    if (!(thresh > 0.0)) return fail(OA_E_BAD_THRESH, "thresh must be > 0 (the reference's make_pairs returns None)");
    if ((rc = refuse_filters_shard(c, "oa_make_pairs"))) return rc;
    if ((rc = use_device(c))) return rc;
    if ((rc = ensure_common(c))) return rc;
    if ((rc = ensure_filters(c))) return rc;
    *K = 0;
    if (dstats) { dstats[0] = NAN; dstats[1] = NAN; }
    if (c->src.ns == 0) return OA_OK;
    const int n_blocks = (c->src.ns + 255) / 256;
    if (c->src.emit_cap < c->src.ns) {
        HIPCHK(dev_malloc(&c->src.d_valid, (size_t)c->src.ns));
        HIPCHK(dev_malloc(&c->src.d_b, sizeof(float) * 3 * (size_t)c->src.ns));
        HIPCHK(dev_malloc(&c->src.d_dist, sizeof(double) * (size_t)c->src.ns));
        HIPCHK(dev_malloc(&c->src.d_counts, sizeof(int) * (size_t)n_blocks));
        HIPCHK(dev_malloc(&c->src.d_offsets, sizeof(long long) * (size_t)(n_blocks + 1)));
        HIPCHK(dev_malloc(&c->src.d_A, sizeof(double) * 3 * (size_t)c->src.ns));
        HIPCHK(dev_malloc(&c->src.d_B, sizeof(double) * 3 * (size_t)c->src.ns));
        c->src.d_pos.reset();
        if (c->parent) HIPCHK(dev_malloc(&c->src.d_pos, sizeof(int) * (size_t)c->src.ns));
        c->src.emit_cap = c->src.ns;
    }
    c->d_pivot0 = 0.0;
    if ((rc = make_pairs_pass(c, thresh))) return rc;
    if (calc_stats) {
        // np.std is two-pass; redo the (cheap) accumulation around the mean of the first pass so that the
        // population std is accurate even when it is tiny compared with the mean
        double s1[oa::NSUMS];
        { int rcr = read_small(c, s1, c->d_sums, sizeof s1); if (rcr) return rcr; }
        if (s1[oa::S_K] > 0.0) {
            c->d_pivot0 = s1[oa::S_D] / s1[oa::S_K];
            if ((rc = make_pairs_pass(c, thresh))) { c->d_pivot0 = 0.0; return rc; }
        }
    }
    hipLaunchKernelGGL(oa::k_block_counts, dim3(n_blocks), dim3(256), 0, c->stream, c->src.d_valid, c->src.ns, c->src.d_counts);
    hipLaunchKernelGGL(oa::k_scan_counts, dim3(1), dim3(1024), 0, c->stream, c->src.d_counts, n_blocks, c->src.d_offsets);
    hipLaunchKernelGGL(oa::k_scatter_pairs, dim3(n_blocks), dim3(256), 0, c->stream, c->src.d_valid, c->src.ns,
                       c->src.d_perm ? c->src.d_src4o : c->src.d_src4,
                       c->src.d_b, c->src.d_offsets, (long long)c->src.ns, c->src.d_A, c->src.d_B, (const int *)c->src.d_members, c->src.shard_begin,
                       c->parent ? c->src.d_pos : (int *)nullptr);
    HIPCHK(hipGetLastError());
    double sums[oa::NSUMS];
    long long total = 0;
    HIPCHK(hipMemcpyAsync(sums, c->d_sums, sizeof sums, hipMemcpyDeviceToHost, c->stream));
    { int rcr = read_small(c, &total, c->src.d_offsets + n_blocks, sizeof total); if (rcr) return rcr; }
    if (total > cap) return fail(OA_E_CAPACITY, "oa_make_pairs: %lld pairs but capacity %lld", total, (long long)cap);
    for (int a = 0; a < 3 && total > 0; ++a) {
        HIPCHK(hipMemcpyAsync(A + (size_t)a * cap, c->src.d_A + (size_t)a * c->src.ns, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(B + (size_t)a * cap, c->src.d_B + (size_t)a * c->src.ns, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    *K = total;
    if (calc_stats && dstats && total > 0) {
        const double kk = sums[oa::S_K];
        const double mean_dd = sums[oa::S_D] / kk;                  // relative to the pivot of the second pass
        double var = sums[oa::S_DD] / kk - mean_dd * mean_dd;
        if (var < 0.0) var = 0.0;
        dstats[0] = mean_dd + c->d_pivot0;                          // np.mean(dists)  (general.py:324)
        dstats[1] = sqrt(var);                                      // np.std(dists)   (general.py:325)
    }
    c->d_pivot0 = 0.0;
    return OA_OK;
}

// ================================================================================================
// contract 2: affine_matrix_from_points (shear=False, usesvd=True)
// ================================================================================================
namespace {
int solve_on_device(oa_ctx *c, const double *d_sums, const double pv[3], int with_scale, double M[16])
{
    hipLaunchKernelGGL(oa::k_solve_only, dim3(1), dim3(64), 0, c->stream, d_sums, pv[0], pv[1], pv[2], with_scale, c->d_solve);
    HIPCHK(hipGetLastError());
    double out[17];
    { int rcr = read_small(c, out, c->d_solve, sizeof out); if (rcr) return rcr; }
    if (out[16] != 1.0) return fail(OA_E_TOO_FEW_PAIRS, "input arrays are of wrong shape or type");
    memcpy(M, out, sizeof(double) * 16);
    return OA_OK;
}
// `rows` rows of K doubles, row a at h + a ld on the host -> a fresh d, row a at d + a K; the copies on the context's stream
int upload_rows(oa_ctx *c, DevTmp<double> &d, const double *h, int rows, int64_t K, int64_t ld)
{
    HIPCHK(d.alloc((size_t)rows * (size_t)K));
    for (int a = 0; a < rows; ++a)
        HIPCHK(hipMemcpyAsync(d.p + (size_t)a * K, h + (size_t)a * ld, sizeof(double) * (size_t)K, hipMemcpyHostToDevice, c->stream));
    return OA_OK;
}
// the end of a plane-row step from caller-supplied pairs (point-to-plane, symmetric): the blocks' partial rows -> their sums -> the
// 6x6 solve -> M and the rank.  Pairs with unusable normals do not count towards the three a step needs.
int plane_step_finish(oa_ctx *c, int blocks, const double pv[3], int symmetric, double M[16])
{
    hipLaunchKernelGGL(oa::k_reduce_partials_plane, dim3(1), dim3(oa::RED_THREADS), 0, c->stream, (const double *)c->d_partials, blocks, c->d_sums);
    hipLaunchKernelGGL(oa::k_solve_only_plane, dim3(1), dim3(64), 0, c->stream, (const double *)c->d_sums, pv[0], pv[1], pv[2], symmetric, c->d_solve);
    HIPCHK(hipGetLastError());
    double out[18];
    { int rcr = read_small(c, out, c->d_solve, sizeof out); if (rcr) return rcr; }
    if (out[16] != 1.0) return fail(OA_E_TOO_FEW_PAIRS, "input arrays are of wrong shape or type");
    memcpy(M, out, sizeof(double) * 16);
    c->last_plane_rank = (int)out[17];
    return OA_OK;
}
}  // namespace

OA_EXPORT int oa_kabsch(oa_ctx *c, const double *A, const double *B, int64_t K, int64_t ld, int with_scale, double M[16])
{
    if (!c || !M) return fail(OA_E_BAD_ARG, "oa_kabsch: null argument");
    OA_ROUTE_FIRST(c, oa_kabsch(sub, A, B, K, ld, with_scale, M));
    if (K < 3) return fail(OA_E_TOO_FEW_PAIRS, "input arrays are of wrong shape or type");   // general.py:150-157
    if (!A || !B || ld < K) return fail(OA_E_BAD_ARG, "oa_kabsch: bad arrays");
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = ensure_common(c))) return rc;
    DevTmp<double> dA, dB;
    if ((rc = upload_rows(c, dA, A, 3, K, ld)) || (rc = upload_rows(c, dB, B, 3, K, ld))) return rc;
    const double pv[3] = { A[0], A[ld], A[2 * ld] };
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(oa::ACC_MAX_BLOCKS, (K + oa::ACC_THREADS - 1) / oa::ACC_THREADS));
    hipLaunchKernelGGL(oa::k_accumulate_pairs, dim3(blocks), dim3(oa::ACC_THREADS), 0, c->stream, (const double *)dA.p,
                       (const double *)dB.p, (long long)K, (long long)K, pv[0], pv[1], pv[2], c->d_partials);
    hipLaunchKernelGGL(oa::k_reduce_partials, dim3(1), dim3(oa::RED_THREADS), 0, c->stream, (const oa::DevState *)nullptr,
                       (const double *)c->d_partials, oa::RowSel{ blocks, 0, 0 }, c->d_sums, (unsigned long long *)nullptr);
    HIPCHK(hipGetLastError());
    rc = solve_on_device(c, c->d_sums, pv, with_scale, M);      // synchronises the stream
    if (rc) (void)hipStreamSynchronize(c->stream);
    return rc;
}

// the plane step from caller-supplied pairs (the plane counterpart of oa_kabsch): k_accumulate_pairs_plane -> k_reduce_partials_plane
// -> k_solve_only_plane.  Does not look at the context's metric.
OA_EXPORT int oa_point_to_plane(oa_ctx *c, const double *A, const double *B, const double *N, int64_t K, int64_t ld, double M[16])
{
    if (!c || !M) return fail(OA_E_BAD_ARG, "oa_point_to_plane: null argument");
    OA_ROUTE_FIRST(c, oa_point_to_plane(sub, A, B, N, K, ld, M));
    if (K < 3) return fail(OA_E_TOO_FEW_PAIRS, "input arrays are of wrong shape or type");   // the point metric's rule (general.py:150-157)
    if (!A || !B || !N || ld < K) return fail(OA_E_BAD_ARG, "oa_point_to_plane: bad arrays");
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = ensure_common(c))) return rc;
    DevTmp<double> dA, dB, dN;
    if ((rc = upload_rows(c, dA, A, 3, K, ld)) || (rc = upload_rows(c, dB, B, 3, K, ld)) || (rc = upload_rows(c, dN, N, 3, K, ld))) return rc;
    const double pv[3] = { A[0], A[ld], A[2 * ld] };
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(oa::ACC_MAX_BLOCKS, (K + oa::ACC_THREADS - 1) / oa::ACC_THREADS));
    hipLaunchKernelGGL(oa::k_accumulate_pairs_plane, dim3(blocks), dim3(oa::ACC_THREADS), 0, c->stream, (const double *)dA.p, (const double *)dB.p,
                       (const double *)dN.p, (long long)K, (long long)K, pv[0], pv[1], pv[2], c->d_partials);
    return plane_step_finish(c, blocks, pv, 0, M);
}

// the symmetric step from caller-supplied pairs (oa_point_to_plane with both sides' normals): k_accumulate_pairs_symm ->
// k_reduce_partials_plane -> k_solve_only_plane.  Does not look at the context's metric.
OA_EXPORT int oa_symmetric_step(oa_ctx *c, const double *A, const double *B, const double *NA, const double *NB, int64_t K, int64_t ld, double M[16])
{
    if (!c || !M) return fail(OA_E_BAD_ARG, "oa_symmetric_step: null argument");
    OA_ROUTE_FIRST(c, oa_symmetric_step(sub, A, B, NA, NB, K, ld, M));
    if (K < 3) return fail(OA_E_TOO_FEW_PAIRS, "input arrays are of wrong shape or type");   // the point metric's rule (general.py:150-157)
    if (!A || !B || !NA || !NB || ld < K) return fail(OA_E_BAD_ARG, "oa_symmetric_step: bad arrays");
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = ensure_common(c))) return rc;
    DevTmp<double> dA, dB, dNA, dNB;
    if ((rc = upload_rows(c, dA, A, 3, K, ld)) || (rc = upload_rows(c, dB, B, 3, K, ld))) return rc;
    if ((rc = upload_rows(c, dNA, NA, 3, K, ld)) || (rc = upload_rows(c, dNB, NB, 3, K, ld))) return rc;
    const double pv[3] = { A[0], A[ld], A[2 * ld] };
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(oa::ACC_MAX_BLOCKS, (K + oa::ACC_THREADS - 1) / oa::ACC_THREADS));
    hipLaunchKernelGGL(oa::k_accumulate_pairs_symm, dim3(blocks), dim3(oa::ACC_THREADS), 0, c->stream, (const double *)dA.p, (const double *)dB.p,
                       (const double *)dNA.p, (const double *)dNB.p, (long long)K, (long long)K, pv[0], pv[1], pv[2], c->d_partials);
    return plane_step_finish(c, blocks, pv, 1, M);
}

// the reference's full signature: any ndims (2..8 on the fixed-size kernels, up to 64 through a device workspace), shear (full
// affine) or rigid / similarity
OA_EXPORT int oa_affine_from_points(oa_ctx *c, const double *v0, const double *v1, int ndims, int64_t K, int64_t ld,
                                    int shear, int with_scale, double *M)
{
    if (!c || !M) return fail(OA_E_BAD_ARG, "oa_affine_from_points: null argument");
    OA_ROUTE_FIRST(c, oa_affine_from_points(sub, v0, v1, ndims, K, ld, shear, with_scale, M));
    if (ndims < 2 || K < ndims) return fail(OA_E_TOO_FEW_PAIRS, "input arrays are of wrong shape or type");   // general.py:150-157
    if (ndims > oa::AFF_MAXD_HEAP) return fail(OA_E_BAD_ARG, "oa_affine_from_points: ndims %d > %d", ndims, oa::AFF_MAXD_HEAP);
    if (!v0 || !v1 || ld < K) return fail(OA_E_BAD_ARG, "oa_affine_from_points: bad arrays");
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = ensure_common(c))) return rc;
    const int n = ndims, w = n + 1;
    if (n > oa::AFF_MAXD) {
        // more than 8 dimensions (no caller in the add-on; the reference's signature takes any): one workgroup per row and per
        // Gram entry, the solve with its matrices in a device workspace
        const int D = n <= 16 ? 16 : (n <= 32 ? 32 : 64), m = 2 * n;
        DevTmp<double> d0, d1, d_cs, d_gram, d_out, d_ws;
        if ((rc = upload_rows(c, d0, v0, n, K, ld)) || (rc = upload_rows(c, d1, v1, n, K, ld))) return rc;
        HIPCHK(d_cs.alloc((size_t)2 * D)); HIPCHK(d_gram.alloc((size_t)m * m)); HIPCHK(d_out.alloc((size_t)w * w + 1));
        HIPCHK(d_ws.alloc(oa::aff_ws_doubles(D)));
        hipLaunchKernelGGL(oa::k_affine_rowsum_any, dim3((unsigned)m), dim3(256), 0, c->stream, (const double *)d0.p, (const double *)d1.p, n, D,
                           (long long)K, (long long)K, d_cs.p);
        hipLaunchKernelGGL(oa::k_affine_gram_any, dim3((unsigned)(m * m)), dim3(256), 0, c->stream, (const double *)d0.p, (const double *)d1.p, n, D,
                           (long long)K, (long long)K, (const double *)d_cs.p, d_gram.p);
        dispatch<64, 16, 32>(D, [&](auto DD) {
            hipLaunchKernelGGL((oa::k_affine_solve<decltype(DD)::value, true>), dim3(1), dim3(64), 0, c->stream, (const double *)d_cs.p, (const double *)d_gram.p, n,
                               (long long)K, shear ? 1 : 0, with_scale ? 1 : 0, d_out.p, d_ws.p);
        });
        HIPCHK(hipGetLastError());
        std::vector<double> out((size_t)w * w + 1);
        { int rcr = read_small(c, out.data(), d_out, sizeof(double) * out.size()); if (rcr) return rcr; }
        if (out[(size_t)w * w] != 1.0) return fail(OA_E_TOO_FEW_PAIRS, "input arrays are of wrong shape or type");
        memcpy(M, out.data(), sizeof(double) * (size_t)w * w);
        return OA_OK;
    }
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(512, (K + 1023) / 1024));
    const long long cols_per_block = ((K + blocks - 1) / blocks + oa::AFF_TILE - 1) / oa::AFF_TILE * oa::AFF_TILE;
    const int gblocks = (int)((K + cols_per_block - 1) / cols_per_block);
    DevTmp<double> d0, d1, p1, p2, d_cs, d_gram, d_out;
    if ((rc = upload_rows(c, d0, v0, n, K, ld)) || (rc = upload_rows(c, d1, v1, n, K, ld))) return rc;
    HIPCHK(p1.alloc((size_t)blocks * oa::AFF_M2)); HIPCHK(p2.alloc((size_t)gblocks * oa::AFF_M2 * oa::AFF_M2));
    HIPCHK(d_cs.alloc(oa::AFF_M2)); HIPCHK(d_gram.alloc(oa::AFF_M2 * oa::AFF_M2)); HIPCHK(d_out.alloc((size_t)w * w + 1));
    hipLaunchKernelGGL(oa::k_affine_colsums, dim3(blocks), dim3(256), 0, c->stream, (const double *)d0.p, (const double *)d1.p, n,
                       (long long)K, (long long)K, p1.p);
    hipLaunchKernelGGL(oa::k_affine_reduce, dim3(1), dim3(64), 0, c->stream, (const double *)p1.p, blocks, oa::AFF_M2, d_cs.p);
    hipLaunchKernelGGL(oa::k_affine_gram, dim3(gblocks), dim3(256), 0, c->stream, (const double *)d0.p, (const double *)d1.p, n,
                       (long long)K, (long long)K, (const double *)d_cs.p, cols_per_block, p2.p);
    hipLaunchKernelGGL(oa::k_affine_reduce, dim3(1), dim3(256), 0, c->stream, (const double *)p2.p, gblocks, oa::AFF_M2 * oa::AFF_M2, d_gram.p);
    hipLaunchKernelGGL((oa::k_affine_solve<oa::AFF_MAXD, false>), dim3(1), dim3(64), 0, c->stream, (const double *)d_cs.p, (const double *)d_gram.p, n,
                       (long long)K, shear ? 1 : 0, with_scale ? 1 : 0, d_out.p, (double *)nullptr);
    HIPCHK(hipGetLastError());
    std::vector<double> out((size_t)w * w + 1);
    { int rcr = read_small(c, out.data(), d_out, sizeof(double) * out.size()); if (rcr) return rcr; }
    if (out[(size_t)w * w] != 1.0) return fail(OA_E_TOO_FEW_PAIRS, "input arrays are of wrong shape or type");
    memcpy(M, out.data(), sizeof(double) * (size_t)w * w);
    return OA_OK;
}

OA_EXPORT int oa_kabsch_from_sums(oa_ctx *c, const double sums[OA_NSUMS], const double pivot[3], int with_scale,
                                  double M[16])
{
    if (!c || !sums || !M) return fail(OA_E_BAD_ARG, "oa_kabsch_from_sums: null argument");
    OA_ROUTE_FIRST(c, oa_kabsch_from_sums(sub, sums, pivot, with_scale, M));
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = ensure_common(c))) return rc;
    const double zero[3] = { 0, 0, 0 };
    HIPCHK(hipMemcpyAsync(c->d_sums, sums, sizeof(double) * oa::NSUMS, hipMemcpyHostToDevice, c->stream));
    return solve_on_device(c, c->d_sums, pivot ? pivot : zero, with_scale, M);
}

// ================================================================================================
// the loop
// ================================================================================================
namespace {
int run_begin(oa_ctx *c, const oa_settings *st)
{
    int rc = begin_loop(c, st, st->iters);
    if (rc) return rc;
    if ((rc = ensure_events(c, std::max(1, st->iters)))) return rc;
    HIPCHK(hipEventRecord(c->ev_loop0, c->stream));
    return OA_OK;
}
// the exchange of the sums between devices and ranks carries OA_NSUMS doubles: the plane metric's wider row does not go through it
// ... and a quantile of the world's residuals needs the world's histogram, not OA_NSUMS doubles.
// `who` (the split-phase loop, or a loop on a multi-device context) cannot carry these rows: the error that says so, or OA_OK
int refuse_wide_row(const oa_ctx *c, const char *who, bool estimated_scale_too = true)
{
    if (const int rc = refuse_filters_multi(c, who)) return rc;
    if (const char *noun = normal_metric_noun(c->metric))
        return fail(OA_E_STATE, "%s: the %s metric runs on a single-device context through oa_run / oa_iterate (call oa_set_metric(ctx, OA_METRIC_POINT) for this path)", who, noun);
    if (estimated_scale_too && auto_scale(c))
        return fail(OA_E_STATE, "%s: a robust scale estimated from the residuals runs on a single-device context through oa_run / oa_iterate (call oa_set_robust_auto(ctx, 0, 0) for this path)", who);
    return OA_OK;
}
}  // namespace

OA_EXPORT int oa_run_begin(oa_ctx *c, const oa_settings *st)
{
    if (!c || !st) return fail(OA_E_BAD_ARG, "oa_run_begin: null argument");
    OA_NOT_MULTI(c, "oa_run_begin (the split-phase loop is for one process per GPU)");
    const int rc = refuse_wide_row(c, "oa_run_begin");
    return rc ? rc : run_begin(c, st);
}

OA_EXPORT int oa_iter_partial(oa_ctx *c, double *d_sums)
{
    if (!c || !d_sums) return fail(OA_E_BAD_ARG, "oa_iter_partial: null argument");
    OA_NOT_MULTI(c, "oa_iter_partial");
    int rc = refuse_wide_row(c, "oa_iter_partial");
    if (rc) return rc;
    if (!c->loop_active) return fail(OA_E_STATE, "oa_iter_partial outside oa_run_begin/oa_run_end");
    if ((rc = use_device(c))) return rc;
    return iter_partial(c, d_sums, true);
}

OA_EXPORT int oa_iter_finish(oa_ctx *c, const double *d_sums)
{
    if (!c || !d_sums) return fail(OA_E_BAD_ARG, "oa_iter_finish: null argument");
    OA_NOT_MULTI(c, "oa_iter_finish");
    int rc = refuse_wide_row(c, "oa_iter_finish", false);       // (the estimated scale is oa_iter_partial's to refuse)
    if (rc) return rc;
    if (!c->loop_active) return fail(OA_E_STATE, "oa_iter_finish outside oa_run_begin/oa_run_end");
    if ((rc = use_device(c))) return rc;
    return iter_finish(c, d_sums);
}

OA_EXPORT int oa_run_end(oa_ctx *c, oa_report *rep)
{
    if (!c || !rep) return fail(OA_E_BAD_ARG, "oa_run_end: null argument");
    OA_NOT_MULTI(c, "oa_run_end");
    int rc = use_device(c);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->ev_loop1, c->stream));
    if ((rc = fill_report(c, rep))) return rc;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev_loop0, c->ev_loop1) == hipSuccess) rep->loop_ms = ms;
    c->loop_active = false;
    return status_error(rep->status);
}

OA_EXPORT int oa_run(oa_ctx *c, const oa_settings *st, oa_report *rep)
{
    if (!c || !st || !rep) return fail(OA_E_BAD_ARG, "oa_run: null argument");
    int rc;
    if (!c->subs.empty()) return (rc = refuse_wide_row(c, "oa_run on a multi-device context")) ? rc : multi_run(c, st, rep);
    if ((rc = run_begin(c, st))) return rc;
    // The whole loop is enqueued ahead of the GPU.  With early exit on, iterations after convergence would still cost
    // three empty launches each (the kernels see DevState.halt and return) -- for a small mesh that converges in 7 of 50
    // iterations, more than the real work.  k_solve_update therefore mirrors the halt flag into a pinned host word,
    // and the host looks at it before it enqueues the next iteration: no copies, nothing added to the stream -- a
    // stale 0 only means a few more empty launches.
    // The host also stays at most `lag` iterations ahead of the GPU (the solve kernel mirrors its iteration counter
    // next to the halt flag): enqueuing is much faster than executing, and a host that is 40 iterations ahead learns
    // about the halt too late to save anything.  Two iterations are always queued, so the GPU never idles.
    // The adaptive grid path (grid_fast_now) needs recent news from the device as well: then the host stays close even
    // when the loop cannot end early.
    bool poll = loop_polls(c, st);
    const int lag = 2;
    volatile int32_t *progress = c->h_poll;
    for (int it = 0; it < st->iters; ++it) {
        if (poll) {
            const auto t_wait = std::chrono::steady_clock::now();
            while (!progress[0] && progress[1] < it - lag) {
                if (std::chrono::steady_clock::now() - t_wait > std::chrono::seconds(5)) { poll = false; break; }   // never hang on a sick GPU; once is enough
                std::this_thread::yield();
            }
            if (progress[0]) break;
        }
        if ((rc = iter_fused(c, true))) { (void)hipStreamSynchronize(c->stream); c->loop_active = false; return rc; }
    }
    return oa_run_end(c, rep);
}

namespace {
bool same_loop_settings(const oa_settings &a, const oa_settings &b)
{
    return a.use_target == b.use_target && a.with_scale == b.with_scale && a.thresh == b.thresh && a.target_d == b.target_d;
}
}  // namespace

// A modal sequence lasts while oa_iterate is called with the same thresh / target_d / use_target / with_scale.  Changed
// settings, or any call that re-stages the device state in between (oa_set_matrices, oa_make_pairs, oa_nn_search,
// oa_run, a new upload), end it: the next oa_iterate starts a new sequence (n = 0, fresh convergence ring) from the
// current matrix_world.
OA_EXPORT int oa_iterate(oa_ctx *c, const oa_settings *st, double M_step[16], double stats[6])
{
    if (!c || !st) return fail(OA_E_BAD_ARG, "oa_iterate: null argument");
    const bool multi = !c->subs.empty();
    int rc;
    if (multi && (rc = refuse_wide_row(c, "oa_iterate on a multi-device context"))) return rc;
    if (c->loop_active && !(c->iterate_mode && same_loop_settings(*st, c->settings))) {
        if (multi) multi_abort(c);
        else { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); c->loop_active = false; }
        if (!multi && (rc = fetch_state(c))) return rc;              // the pose reached so far is where the new sequence starts
        if (multi) for (oa_ctx *sub : c->subs) { if ((rc = use_device(sub))) return rc; if ((rc = fetch_state(sub))) return rc; }
    }
    if (!c->loop_active) {
        if ((rc = multi ? multi_begin(c, st, ITERATE_OPEN) : begin_loop(c, st, ITERATE_OPEN))) return rc;
        c->iterate_mode = true;
        for (oa_ctx *sub : c->subs) sub->iterate_mode = true;       // oa_get_history reads the first child's ring
    }
    oa_ctx *c0 = multi ? c->subs[0] : c;
    if (multi) {
        for (oa_ctx *sub : c->subs) sub->ev_used = 0;
        const bool rccl = c->xch->mode == OA_EXCHANGE_RCCL;             // then the wait is the watchdog's (multi_wait), not fetch_state's
        rc = multi_for_groups(c, [c, rccl](size_t g) -> int {            // every GPU's host thread: one iteration, then the state
            int rg = multi_iteration_group(c, c->groups[g], false);
            for (int i : c->groups[g]) { if (rg || rccl) break; oa_ctx *sub = c->subs[(size_t)i]; if (!(rg = use_device(sub))) rg = fetch_state(sub); }
            return rg;
        });
        if (rc) { const std::string keep = g_err; multi_abort(c, true); g_err = keep; return rc; }
        if (rccl) {
            if ((rc = multi_wait(c))) { for (oa_ctx *sub : c->subs) sub->loop_active = false; c->loop_active = false; return rc; }
            for (oa_ctx *sub : c->subs) { if ((rc = use_device(sub))) return rc; if ((rc = fetch_state(sub))) return rc; }
        }
    } else {
        if ((rc = use_device(c))) return rc;
        c->ev_used = 0;
        if ((rc = iter_fused(c, false))) { (void)hipStreamSynchronize(c->stream); c->loop_active = false; return rc; }
        if ((rc = fetch_state(c))) return rc;
    }
    const oa::DevState &s = c0->h_state;
    if (s.status != 0) {
        if (multi) multi_abort(c); else c->loop_active = false;
        if ((rc = status_error(s.status))) return rc;
        return fail(OA_E_HIP, "oa_iterate: device status %d", s.status);
    }
    if (s.n <= 0) return fail(OA_E_STATE, "oa_iterate: loop already halted");
    oa::StepRecord r;
    memcpy(&r, c0->h_hist_map + ((s.n - 1) % c0->max_records), sizeof r);           // fetch_state synchronised the stream
    if (M_step) memcpy(M_step, r.M, sizeof r.M);
    if (stats) {
        stats[0] = r.K; stats[1] = s.use_target ? r.mean_d : NAN; stats[2] = s.use_target ? r.std_d : NAN;
        stats[3] = r.trans; stats[4] = r.angle; stats[5] = (double)s.converged;
    }
    return OA_OK;
}

OA_EXPORT int oa_get_history(oa_ctx *c, int32_t max_n, double *step_M, float *step_new, int64_t *step_K,
                             double *step_stats, double *step_trans)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    OA_ROUTE_FIRST(c, oa_get_history(sub, max_n, step_M, step_new, step_K, step_stats, step_trans));
    if (use_device(c)) return OA_E_HIP;
    const int total = c->h_state.n, cap = c->max_records;
    const int held = std::min(total, cap);
    const int n = std::min(held, (int)max_n);
    if (n <= 0) return 0;
    std::vector<oa::StepRecord> h_local;
    if (!(c->h_hist_valid && (int)c->h_hist.size() >= held)) {
        h_local.resize((size_t)held);
        if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(OA_E_HIP, "oa_get_history: stream error");
        memcpy(h_local.data(), c->h_hist_map, sizeof(oa::StepRecord) * (size_t)held);
    }
    const std::vector<oa::StepRecord> &h = h_local.empty() ? c->h_hist : h_local;
    // a loop that fits the history: its first n iterations; a ring that wrapped (oa_iterate): the last n, oldest first
    const int first = (total > cap || c->iterate_mode) ? total - n : 0;
    for (int i = 0; i < n; ++i) {
        const oa::StepRecord &r = h[(size_t)((first + i) % cap)];
        if (step_M) memcpy(step_M + 16 * i, r.M, sizeof r.M);
        if (step_new) memcpy(step_new + 16 * i, r.new_mat, sizeof r.new_mat);
        if (step_K) step_K[i] = (int64_t)r.K;
        if (step_stats) { step_stats[2 * i] = r.mean_d; step_stats[2 * i + 1] = r.std_d; }
        if (step_trans) step_trans[i] = r.trans;
    }
    return n;
}

// ================================================================================================
// coarse global alignment (EXTENSION): batched pose scoring, candidates, multi-start refinement (oa_pose.hpp)
// ================================================================================================
namespace {
// what the launches of one call share: the sample list, the base matrices, the call's own thresh and search radius
struct PoseJob {
    oa::PoseBase pb{};
    DevTmp<int> sample;
    int S = 0;
    bool tri = false;
};

// workgroups per pose: enough to fill the chip over all poses, at most one per POSE_WPB sample points
inline int pose_bpp(const oa_ctx *c, int n_poses, int S)
{
    const int want = (c->n_cu * 16 + n_poses - 1) / n_poses;
    const int per = (S + oa::POSE_WPB - 1) / oa::POSE_WPB;
    return std::max(1, std::min(want, std::min(per, oa::POSE_MAX_BPP)));
}

int pose_job_begin(oa_ctx *c, double thresh, int32_t stride, PoseJob &job)
{
    job.tri = c->tgt.surface;
    const bool tree = job.tri ? (c->tgt.tbvh_ok && c->tgt.d_tbvh_box && c->tgt.d_tbvh_prims && c->tgt.d_tri9) : (c->tgt.bvh_ok && c->tgt.d_bvh_box && c->tgt.d_bvh_prims);
    if (!tree) return fail(OA_E_STATE, "pose scoring searches through the target's box tree: none was built (OA_SEARCH_BRUTE, or a target with non-finite coordinates)");
    if (c->src.ns <= 0) return fail(OA_E_STATE, "pose scoring: the selection is empty");
    const int step = stride > 1 ? stride : 1;
    job.S = (c->src.ns + step - 1) / step;
    const oa::DevState &s = c->h_state;
    memcpy(job.pb.mx2, s.mx2, sizeof s.mx2);
    memcpy(job.pb.imx2, s.imx2, sizeof s.imx2);
    job.pb.mx2_identity = mx2_identity(c, s.mx2);
    job.pb.thresh = thresh;
    job.pb.cut_a = INFINITY; job.pb.cut_b = 0.0;
    double lpw = 0.0;
    search_radius(c, s.mx2, thresh, job.pb.cut_a, job.pb.cut_b, lpw);
    for (int k = 0; k < 3; ++k) job.pb.pivot[k] = c->src.pivot[k];
    HIPCHK(job.sample.alloc((size_t)job.S));
    hipLaunchKernelGGL(oa::k_pose_sample, dim3((unsigned)((c->src.ns + 255) / 256)), dim3(256), 0, c->stream, (const int *)c->src.d_perm, c->src.ns, step, job.sample.p);
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// rows: n_poses x bpp rows of NSUMS (full) / POSE_NSCORE doubles
int pose_launch(oa_ctx *c, const PoseJob &job, bool full, const float *d_poses, const float *d_iposes, int n_poses, int bpp, double *d_rows)
{
    const dim3 grid((unsigned)((long long)n_poses * bpp)), block(oa::POSE_WPB * 64);
    auto launch = [&](auto TRI, auto FULL) {
        constexpr bool tri = decltype(TRI)::value;
        hipLaunchKernelGGL((oa::k_pose_score<tri, decltype(FULL)::value>), grid, block, 0, c->stream, job.pb, d_poses, d_iposes, (const float4 *)c->src.d_src4,
                           (const int *)job.sample.p, job.S, bpp, tri ? c->tgt.tbvh : c->tgt.bvh, (const float4 *)(tri ? c->tgt.d_tbvh_box : c->tgt.d_bvh_box),
                           (const float4 *)(tri ? c->tgt.d_tbvh_prims : c->tgt.d_bvh_prims), (const float4 *)c->tgt.d_tri9, d_rows);
    };
    if (job.tri) { if (full) launch(std::true_type{}, std::true_type{}); else launch(std::true_type{}, std::false_type{}); }
    else { if (full) launch(std::false_type{}, std::true_type{}); else launch(std::false_type{}, std::false_type{}); }
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// scores of n_poses poses in device memory: n_poses x OA_POSE_NSCORE {K, mean_dist, std_dist, cost}
int pose_scores(oa_ctx *c, const PoseJob &job, const float *d_poses, int n_poses, double *scores)
{
    const int bpp = pose_bpp(c, n_poses, job.S);
    DevTmp<double> rows, sums;
    HIPCHK(rows.alloc((size_t)n_poses * bpp * oa::POSE_NSCORE));
    HIPCHK(sums.alloc((size_t)n_poses * oa::POSE_NSCORE));
    int rc = pose_launch(c, job, false, d_poses, nullptr, n_poses, bpp, rows.p);
    if (rc) return rc;
    hipLaunchKernelGGL(oa::k_pose_rows_sum, dim3((unsigned)n_poses), dim3(64), 0, c->stream, (const double *)rows.p, bpp, oa::POSE_NSCORE, sums.p);
    HIPCHK(hipGetLastError());
    std::vector<double> h((size_t)n_poses * oa::POSE_NSCORE);
    if ((rc = read_small(c, h.data(), sums.p, sizeof(double) * h.size()))) return rc;
    const double S = (double)job.S;
    for (int p = 0; p < n_poses; ++p) {
        const double K = h[3 * (size_t)p], sd = h[3 * (size_t)p + 1], sdd = h[3 * (size_t)p + 2];
        double *o = scores + (size_t)OA_POSE_NSCORE * p;
        o[0] = K; o[1] = NAN; o[2] = NAN;
        if (K > 0.0) {
            const double mean = sd / K;
            double var = sdd / K - mean * mean;
            if (var < 0.0) var = 0.0;
            o[1] = mean; o[2] = sqrt(var);
        }
        o[3] = K > 0.0 ? (sd + (S - K) * job.pb.thresh) / S : job.pb.thresh;   // (no pair: thresh itself, not S thresh / S)
    }
    return OA_OK;
}

// sum of M @ v over n points (float32 m4_mul_v3 images, fp64 sums, fixed order) -> their centroid
template <int STRIDE>
int centroid_of(oa_ctx *c, const float *d_pts, int n, const float *M, double out[3], const char *what)
{
    const int blocks = std::max(1, std::min(1024, (n + 255) / 256));
    DevTmp<double> rows, sum;
    HIPCHK(rows.alloc((size_t)blocks * 4));
    HIPCHK(sum.alloc(4));
    oa::Mat4f mx;
    memcpy(mx.m, M, sizeof mx.m);
    hipLaunchKernelGGL((oa::k_centroid_rows<STRIDE>), dim3((unsigned)blocks), dim3(256), 0, c->stream, d_pts, n, mx, rows.p);
    hipLaunchKernelGGL(oa::k_pose_rows_sum, dim3(1), dim3(64), 0, c->stream, (const double *)rows.p, blocks, 4, sum.p);
    HIPCHK(hipGetLastError());
    double h[4];
    const int rc = read_small(c, h, sum.p, sizeof h);
    if (rc) return rc;
    if (!(h[3] > 0.0)) return fail(OA_E_STATE, "%s has no finite point", what);
    for (int k = 0; k < 3; ++k) out[k] = h[k] / h[3];
    return OA_OK;
}

void mul4d(const double *A, const double *B, double *out)
{
    double r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double a = 0.0;
            for (int k = 0; k < 4; ++k) a += A[4 * i + k] * B[4 * k + j];
            r[4 * i + j] = a;
        }
    memcpy(out, r, sizeof r);
}

// candidate k = float32(T(c_t) R_k T(-c_s) mx_align), R_k = rotation k of the n_rot-point super-Fibonacci set (Alexa 2022)
int coarse_candidates(oa_ctx *c, int n_rot, float *out)
{
    double cs[3], ct[3];
    int rc = centroid_of<4>(c, (const float *)c->src.d_src4, c->src.ns, c->h_state.mx1, cs, "oa_coarse_candidates: the selection");
    if (rc) return rc;
    if ((rc = centroid_of<3>(c, c->tgt.d_tgt_xyz, c->tgt.nt, c->h_state.mx2, ct, "oa_coarse_candidates: the target"))) return rc;
    double A[16], Tt[16] = { 1, 0, 0, ct[0], 0, 1, 0, ct[1], 0, 0, 1, ct[2], 0, 0, 0, 1 }, Ts[16] = { 1, 0, 0, -cs[0], 0, 1, 0, -cs[1], 0, 0, 1, -cs[2], 0, 0, 0, 1 };
    for (int k = 0; k < 16; ++k) A[k] = (double)c->h_state.mx1[k];
    double right[16];
    mul4d(Ts, A, right);
    const double two_pi = 6.283185307179586476925286766559, psi = 1.533751168755204288118041;
    for (int k = 0; k < n_rot; ++k) {
        const double s = (double)k + 0.5, t = s / (double)n_rot;
        const double r = sqrt(t), R = sqrt(1.0 - t), alpha = two_pi * s / sqrt(2.0), beta = two_pi * s / psi;
        const double x = r * sin(alpha), y = r * cos(alpha), z = R * sin(beta), w = R * cos(beta);
        const double Rm[16] = { 1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w), 0.0,
                                2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w), 0.0,
                                2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y), 0.0,
                                0.0, 0.0, 0.0, 1.0 };
        double M[16];
        mul4d(Rm, right, M);
        mul4d(Tt, M, M);
        for (int e = 0; e < 16; ++e) out[16 * (size_t)k + e] = (float)M[e];
    }
    return OA_OK;
}

int pose_call_ready(oa_ctx *c)
{
    int rc = check_ready(c);
    if (rc) return rc;
    if ((rc = use_device(c))) return rc;
    return ensure_common(c);
}
}  // namespace

OA_EXPORT int oa_score_poses(oa_ctx *c, const float *mx_align, int32_t n_poses, double thresh, int32_t stride, double *scores)
{
    if (!c || !mx_align || !scores) return fail(OA_E_BAD_ARG, "oa_score_poses: null argument");
    OA_NOT_MULTI(c, "oa_score_poses");
    int rc = pose_call_ready(c);
    if (rc) return rc;
    if (!(thresh > 0.0)) return fail(OA_E_BAD_THRESH, "thresh must be > 0 (the reference's make_pairs returns None)");
    if (!(thresh < INFINITY)) return fail(OA_E_BAD_ARG, "oa_score_poses: thresh must be finite");
    if (n_poses < 1 || n_poses > 65536) return fail(OA_E_BAD_ARG, "oa_score_poses: %d poses (1 .. 65536)", n_poses);
    for (size_t k = 0; k < 16 * (size_t)n_poses; ++k)
        if (!(fabsf(mx_align[k]) < INFINITY)) return fail(OA_E_BAD_ARG, "oa_score_poses: entry %zu of pose %zu is not finite", k % 16, k / 16);
    {
        const long long step = stride > 1 ? stride : 1, S = (c->src.ns + step - 1) / step;
        if (S * n_poses >= (1ll << 31)) return fail(OA_E_BAD_ARG, "oa_score_poses: %lld sample points x %d poses: 2^31 queries or more", S, n_poses);
    }
    PoseJob job;
    if ((rc = pose_job_begin(c, thresh, stride, job))) return rc;
    DevTmp<float> d_poses;
    HIPCHK(d_poses.alloc(16 * (size_t)n_poses));
    HIPCHK(hipMemcpyAsync(d_poses.p, mx_align, sizeof(float) * 16 * (size_t)n_poses, hipMemcpyHostToDevice, c->stream));
    rc = pose_scores(c, job, d_poses.p, n_poses, scores);
    if (rc) (void)hipStreamSynchronize(c->stream);                // (the caller's matrices may still be on their way)
    return rc;
}

OA_EXPORT int oa_coarse_candidates(oa_ctx *c, int32_t n_rot, float *mx_align_out)
{
    if (!c || !mx_align_out) return fail(OA_E_BAD_ARG, "oa_coarse_candidates: null argument");
    OA_NOT_MULTI(c, "oa_coarse_candidates");
    int rc = pose_call_ready(c);
    if (rc) return rc;
    if (n_rot < 1 || n_rot > 65536) return fail(OA_E_BAD_ARG, "oa_coarse_candidates: %d rotations (1 .. 65536)", n_rot);
    if (c->src.ns <= 0) return fail(OA_E_STATE, "oa_coarse_candidates: the selection is empty");
    return coarse_candidates(c, n_rot, mx_align_out);
}

namespace {
// what oa_coarse_align and oa_coarse_align_poses check first
int coarse_call_begin(oa_ctx *c, const char *who, const oa_coarse_settings *cs, oa_coarse_report *rep, bool uses_n_rot)
{
    int rc = pose_call_ready(c);
    if (rc) return rc;
    if (!(cs->thresh > 0.0)) return fail(OA_E_BAD_THRESH, "thresh must be > 0 (the reference's make_pairs returns None)");
    if (!(cs->thresh < INFINITY) || (uses_n_rot && (cs->n_rot < 1 || cs->n_rot > 65536)) || cs->n_refine < 1 || cs->n_refine > 4096 || cs->refine_iters < 0 || cs->refine_iters > 10000)
        return fail(OA_E_BAD_ARG, "%s: n_rot 1 .. 65536, n_refine 1 .. 4096, refine_iters 0 .. 10000 and a finite thresh", who);
    memset(rep, 0, sizeof *rep);
    // the call ends a running sequence, as oa_set_matrices does; the pose it reached is the incoming one
    if (c->loop_active) {
        if ((rc = fetch_state(c))) return rc;
        c->loop_active = false;
    }
    return OA_OK;
}

// The multi-start recipe over cand = n_rot candidates followed by the incoming pose (P = n_rot + 1 matrices): one scoring launch,
// the n_refine best refined, rescored, matrix_world <- the lowest cost (or left alone).  t0: when the call began.
int coarse_align_body(oa_ctx *c, const char *who, const oa_coarse_settings *cs, oa_coarse_report *rep, const std::vector<float> &cand, int n_rot,
                      std::chrono::steady_clock::time_point t0)
{
    int rc = OA_OK;
    auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    const int P = n_rot + 1;                                        // the incoming pose is candidate n_rot
    const int n_ref = std::min((int)cs->n_refine, P);
    {
        const long long step = cs->stride > 1 ? cs->stride : 1, S = (c->src.ns + step - 1) / step;
        if (S * P >= (1ll << 31)) return fail(OA_E_BAD_ARG, "%s: %lld sample points x %d poses: 2^31 queries or more", who, S, P);
    }
    PoseJob job;
    if ((rc = pose_job_begin(c, cs->thresh, cs->stride, job))) return rc;
    DevTmp<float> d_poses, d_iposes;
    HIPCHK(d_poses.alloc(16 * (size_t)P));
    HIPCHK(hipMemcpyAsync(d_poses.p, cand.data(), sizeof(float) * cand.size(), hipMemcpyHostToDevice, c->stream));
    std::vector<double> sc((size_t)OA_POSE_NSCORE * P);
    const auto t1 = std::chrono::steady_clock::now();
    if ((rc = pose_scores(c, job, d_poses.p, P, sc.data()))) { (void)hipStreamSynchronize(c->stream); return rc; }
    rep->score_ms = ms_since(t1);
    // the n_refine lowest costs, ties to the lower index; the incoming pose is always among them
    std::vector<int> order((size_t)P);
    for (int k = 0; k < P; ++k) order[(size_t)k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sc[4 * (size_t)a + 3] < sc[4 * (size_t)b + 3]; });
    std::vector<int> pick(order.begin(), order.begin() + n_ref);
    if (std::find(pick.begin(), pick.end(), n_rot) == pick.end()) pick.back() = n_rot;
    std::vector<float> ref(16 * (size_t)n_ref), iref(16 * (size_t)n_ref);
    for (int k = 0; k < n_ref; ++k) {
        memcpy(&ref[16 * (size_t)k], &cand[16 * (size_t)pick[(size_t)k]], sizeof(float) * 16);
        if (!oa::m4_inverted(&ref[16 * (size_t)k], &iref[16 * (size_t)k])) return fail(OA_E_SINGULAR, "%s: candidate %d has no inverse", who, pick[(size_t)k]);
    }
    HIPCHK(d_iposes.alloc(16 * (size_t)n_ref));
    HIPCHK(hipStreamSynchronize(c->stream));                      // (d_poses is reused: the first upload has been read)
    HIPCHK(hipMemcpyAsync(d_poses.p, ref.data(), sizeof(float) * ref.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_iposes.p, iref.data(), sizeof(float) * iref.size(), hipMemcpyHostToDevice, c->stream));
    if (cs->refine_iters > 0) {
        const int bpp = pose_bpp(c, n_ref, job.S);
        DevTmp<double> rows;
        HIPCHK(rows.alloc((size_t)n_ref * bpp * oa::NSUMS));
        for (int it = 0; it < cs->refine_iters; ++it) {
            if ((rc = pose_launch(c, job, true, d_poses.p, d_iposes.p, n_ref, bpp, rows.p))) { (void)hipStreamSynchronize(c->stream); return rc; }
            hipLaunchKernelGGL(oa::k_pose_solve, dim3((unsigned)n_ref), dim3(64), 0, c->stream, (const double *)rows.p, bpp, c->src.pivot[0], c->src.pivot[1], c->src.pivot[2],
                               d_poses.p, d_iposes.p);
            HIPCHK(hipGetLastError());
        }
    }
    std::vector<double> sr((size_t)OA_POSE_NSCORE * n_ref);
    if ((rc = pose_scores(c, job, d_poses.p, n_ref, sr.data()))) { (void)hipStreamSynchronize(c->stream); return rc; }
    if ((rc = read_small(c, ref.data(), d_poses.p, sizeof(float) * ref.size()))) return rc;
    int win = 0;
    for (int k = 1; k < n_ref; ++k) if (sr[4 * (size_t)k + 3] < sr[4 * (size_t)win + 3]) win = k;
    const double cost_start = sc[4 * (size_t)n_rot + 3];
    rep->n_candidates = n_rot;
    rep->cost_start = cost_start;
    float inv[16];
    const bool better = sr[4 * (size_t)win + 3] < cost_start && oa::m4_inverted(&ref[16 * (size_t)win], inv);
    const int origin = better ? pick[(size_t)win] : n_rot;
    rep->best_candidate = origin;
    rep->best_rank = (int32_t)(std::find(order.begin(), order.end(), origin) - order.begin());
    rep->cost_best_candidate = sc[4 * (size_t)origin + 3];
    if (better) {
        rep->cost_refined = sr[4 * (size_t)win + 3];
        rep->K_refined = (int64_t)sr[4 * (size_t)win];
        memcpy(c->h_state.mx1, &ref[16 * (size_t)win], sizeof inv);
        memcpy(c->h_state.imx1, inv, sizeof inv);
        c->last_todo_wave_max = -1;                                 // a new pose (oa_set_matrices)
    } else {                                                        // nothing beats the incoming pose: it stays in force
        rep->cost_refined = cost_start;
        rep->K_refined = (int64_t)sc[4 * (size_t)n_rot];
    }
    rep->status = OA_OK;
    rep->total_ms = ms_since(t0);
    return OA_OK;
}
}  // namespace

OA_EXPORT int oa_coarse_align(oa_ctx *c, const oa_coarse_settings *cs, oa_coarse_report *rep)
{
    if (!c || !cs || !rep) return fail(OA_E_BAD_ARG, "oa_coarse_align: null argument");
    OA_NOT_MULTI(c, "oa_coarse_align");
    int rc = coarse_call_begin(c, "oa_coarse_align", cs, rep, true);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const int n_rot = cs->n_rot;
    std::vector<float> cand(16 * ((size_t)n_rot + 1));
    if ((rc = coarse_candidates(c, n_rot, cand.data()))) return rc;
    memcpy(cand.data() + 16 * (size_t)n_rot, c->h_state.mx1, sizeof(float) * 16);
    return coarse_align_body(c, "oa_coarse_align", cs, rep, cand, n_rot, t0);
}

OA_EXPORT int oa_coarse_align_poses(oa_ctx *c, const float *mx_align, int32_t n_poses, const oa_coarse_settings *cs, oa_coarse_report *rep)
{
    if (!c || !mx_align || !cs || !rep) return fail(OA_E_BAD_ARG, "oa_coarse_align_poses: null argument");
    OA_NOT_MULTI(c, "oa_coarse_align_poses");
    int rc = coarse_call_begin(c, "oa_coarse_align_poses", cs, rep, false);
    if (rc) return rc;
    if (n_poses < 1 || n_poses > 65535) return fail(OA_E_BAD_ARG, "oa_coarse_align_poses: %d poses (1 .. 65535)", n_poses);
    for (size_t k = 0; k < 16 * (size_t)n_poses; ++k)
        if (!(fabsf(mx_align[k]) < INFINITY)) return fail(OA_E_BAD_ARG, "oa_coarse_align_poses: entry %zu of pose %zu is not finite", k % 16, k / 16);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<float> cand(16 * ((size_t)n_poses + 1));
    memcpy(cand.data(), mx_align, sizeof(float) * 16 * (size_t)n_poses);
    memcpy(cand.data() + 16 * (size_t)n_poses, c->h_state.mx1, sizeof(float) * 16);
    return coarse_align_body(c, "oa_coarse_align_poses", cs, rep, cand, n_poses, t0);
}

// ================================================================================================
// k nearest target vertices / PCA normals of a point-cloud target (EXTENSION; oa_knn.hpp)
// ================================================================================================
namespace {
// the vertex tree a k-nearest call walks: the context's own when it has one, else a tree of the call's own (OA_SEARCH_BRUTE
// skips the build with the upload; a target with non-finite coordinates has no bounding box -- its tree is laid out over
// the box of the finite coordinates, the others sit in leaves whose boxes ignore them)
struct KnnTree {
    oa::BvhParams bp{};
    const float4 *box = nullptr, *prims = nullptr;
    DevBuf<float4> own_box, own_prims;
};

// the box of the target's finite coordinates, base-local (all zero when there is none)
int target_bbox(oa_ctx *c, double lo[3], double hi[3])
{
    for (int a = 0; a < 3; ++a) { lo[a] = 0.0; hi[a] = 0.0; }
    if (c->tgt.filter_ok) { for (int a = 0; a < 3; ++a) { lo[a] = c->bb_lo[a]; hi[a] = c->bb_hi[a]; } return OA_OK; }
    const int nb = 256;
    DevTmp<float> d_bb;
    HIPCHK(d_bb.alloc(6 * (size_t)nb));
    hipLaunchKernelGGL(oa::k_bbox_finite, dim3(nb), dim3(256), 0, c->stream, (const float *)c->tgt.d_tgt_xyz, c->tgt.nt, d_bb.p);
    HIPCHK(hipGetLastError());
    std::vector<float> bb(6 * (size_t)nb);
    const int rc = read_small(c, bb.data(), d_bb.p, sizeof(float) * bb.size());
    if (rc) return rc;
    float l[3], h[3];
    (void)fold_bbox(bb.data(), nb, l, h);                            // (k_bbox_finite leaves the non-finite coordinates out)
    for (int a = 0; a < 3; ++a) if (l[a] <= h[a]) { lo[a] = l[a]; hi[a] = h[a]; }     // (no finite coordinate: any frame will do)
    return OA_OK;
}

// Where a call writes the target normals it computes.  install: the target's own array, allocated on first use -- the stream
// carries this call alone, so the array the loops read is replaced in place, and a boundary mask built from the old normals no
// longer holds.  Else `tmp` when the caller wants them (wanted), else nowhere (d_n stays null).
int new_normals_dest(oa_ctx *c, int install, bool wanted, DevTmp<float> &tmp, float *&d_n)
{
    const size_t nt = (size_t)c->tgt.nt;
    if (install) {
        if (!c->tgt.d_tgt_n) HIPCHK(dev_malloc(&c->tgt.d_tgt_n, sizeof(float) * 3 * nt));
        c->tgt.bnd_ok = false;
        d_n = c->tgt.d_tgt_n;
    } else if (wanted) { HIPCHK(tmp.alloc(3 * nt)); d_n = tmp.p; }
    return OA_OK;
}

int knn_tree(oa_ctx *c, KnnTree &t)
{
    if (c->tgt.bvh_ok && c->tgt.d_bvh_box && c->tgt.d_bvh_prims) { t.bp = c->tgt.bvh; t.box = c->tgt.d_bvh_box; t.prims = c->tgt.d_bvh_prims; return OA_OK; }
    double lo[3], hi[3];
    { const int rcb = target_bbox(c, lo, hi); if (rcb) return rcb; }
    bool ok = false;
    const int rc = build_bvh_arrays(c, false, c->tgt.d_tgt_xyz, 3, c->tgt.nt, lo, hi, t.bp, t.own_box, t.own_prims, ok);
    if (rc) return rc;
    if (!ok) return fail(OA_E_CAPACITY, "the target's box tree would need more than %d levels", oa::BVH_MAX_LEVELS);
    t.box = t.own_box; t.prims = t.own_prims;
    return OA_OK;
}

// What every call on a point-cloud target checks and does first; a running sequence ends the way oa_set_target_normals ends
// one.  what: the sentence a surface target gets.  k_min > 0: the call takes a k, k_min .. min(KNN_MAX_K, nt), refused after the
// target and before the device is touched, so that a refused call leaves a running sequence alone.
enum class CloudCall { NEIGHBOURS, STRAYS };
int cloud_call_begin(oa_ctx *c, const char *who, CloudCall what, int k = 0, int k_min = 0)
{
    if (c->tgt.nt <= 0) return fail(OA_E_STATE, "%s: call oa_set_target first", who);
    if (c->tgt.surface && what == CloudCall::NEIGHBOURS) return fail(OA_E_STATE, "%s: a surface target (oa_set_target_mesh) uses its triangles' geometric normals", who);
    if (c->tgt.surface) return fail(OA_E_STATE, "%s: a surface target (oa_set_target_mesh) has no stray vertices to look for; upload a cloud", who);
    if (k_min > 0 && (k < k_min || k > oa::KNN_MAX_K || k > c->tgt.nt))
        return fail(OA_E_BAD_ARG, "%s: k = %d outside %d .. min(%d, %d target vertices)", who, k, k_min, oa::KNN_MAX_K, c->tgt.nt);
    const int rc = use_device(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->loop_active = false;
    return OA_OK;
}

// workgroups of a grid-stride launch that deals `items` (leaves of the vertex tree, vertices) to waves, per_block to a workgroup
inline unsigned wave_blocks(const oa_ctx *c, int items, int per_block) { return (unsigned)std::max(1, std::min((items + per_block - 1) / per_block, c->n_cu * 32)); }

// the point a sign rule looks toward or away from: the caller's, or (null) the centroid of the target's finite vertices
int orient_point_or_centroid(oa_ctx *c, const char *who, const float point[3], double out[3])
{
    if (point) { for (int a = 0; a < 3; ++a) out[a] = (double)point[a]; return OA_OK; }
    return centroid_of<3>(c, c->tgt.d_tgt_xyz, c->tgt.nt, EYE16, out, (std::string(who) + ": the target").c_str());
}

// the squared radius a limited search compares against: the float32 square of the float32 setting, rounded once
// (radius_count_launch's constant); +inf while the setting is off
inline float neighbor_r2(const oa_ctx *c) { return c->nbr_radius > 0.f ? c->nbr_radius * c->nbr_radius : INFINITY; }

// r2: neighbor_r2(c) for the calls the setting limits, +inf for those it does not (oa_orient_target_normals)
template <bool PCA>
int knn_launch(oa_ctx *c, const KnnTree &t, int k, float r2, int32_t *d_idx, float *d_d2, const oa::KnnOrient &orient, float *d_n, float *d_curv)
{
    const int wpb = oa::knn_waves_per_block(k);
    hipLaunchKernelGGL((oa::k_bvh_knn<PCA>), dim3(wave_blocks(c, t.bp.cnt[1], wpb)), dim3(64 * wpb), 0, c->stream, t.bp, t.box, t.prims, k, r2, d_idx, d_d2,
                       (const float *)c->tgt.d_tgt_xyz, orient, d_n, d_curv);
    HIPCHK(hipGetLastError());
    return OA_OK;
}
}  // namespace

OA_EXPORT int oa_target_knn(oa_ctx *c, int k, int32_t *out_idx, float *out_d2)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (!c->subs.empty() && c->loop_active) multi_abort(c);
    // (the target is replicated: every child computes the same bits; the first one's go out)
    OA_ROUTE_ALL_PAR(c, oa_target_knn(sub, k, sub->rank == 0 ? out_idx : nullptr, sub->rank == 0 ? out_d2 : nullptr));
    int rc = cloud_call_begin(c, "oa_target_knn", CloudCall::NEIGHBOURS, k, 1);
    if (rc) return rc;
    KnnTree tree;
    if ((rc = knn_tree(c, tree))) return rc;
    const size_t n = (size_t)c->tgt.nt * (size_t)k;
    DevTmp<int32_t> d_idx;
    DevTmp<float> d_d2;
    if (out_idx) HIPCHK(d_idx.alloc(n));
    if (out_d2) HIPCHK(d_d2.alloc(n));
    if ((rc = knn_launch<false>(c, tree, k, neighbor_r2(c), d_idx.p, d_d2.p, oa::KnnOrient{}, nullptr, nullptr))) return rc;
    if (out_idx) HIPCHK(hipMemcpyAsync(out_idx, d_idx.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    if (out_d2) HIPCHK(hipMemcpyAsync(out_d2, d_d2.p, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return OA_OK;
}

OA_EXPORT int oa_estimate_target_normals(oa_ctx *c, int k, int orient, const float orient_point[3], int install, float *out_normals,
                                         float *out_curvature)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    if (orient != OA_ORIENT_NONE && orient != OA_ORIENT_TOWARD && orient != OA_ORIENT_AWAY)
        return fail(OA_E_BAD_ARG, "oa_estimate_target_normals: orient %d (use OA_ORIENT_NONE / OA_ORIENT_TOWARD / OA_ORIENT_AWAY)", orient);
    if (orient == OA_ORIENT_TOWARD && !orient_point) return fail(OA_E_BAD_ARG, "oa_estimate_target_normals: OA_ORIENT_TOWARD needs a point");
    if (!c->subs.empty() && c->loop_active) multi_abort(c);
    OA_ROUTE_ALL_PAR(c, oa_estimate_target_normals(sub, k, orient, orient_point, install, sub->rank == 0 ? out_normals : nullptr,
                                                   sub->rank == 0 ? out_curvature : nullptr));
    static const char who[] = "oa_estimate_target_normals";
    int rc = cloud_call_begin(c, who, CloudCall::NEIGHBOURS, k, 3);
    if (rc) return rc;
    KnnTree tree;
    if ((rc = knn_tree(c, tree))) return rc;
    oa::KnnOrient ko{};
    ko.mode = orient;
    if (orient != OA_ORIENT_NONE && (rc = orient_point_or_centroid(c, who, orient_point, ko.p))) return rc;
    const size_t nt = (size_t)c->tgt.nt;
    DevTmp<float> tmp_n, d_curv;
    float *d_n = nullptr;
    if ((rc = new_normals_dest(c, install, out_normals != nullptr, tmp_n, d_n))) return rc;
    if (out_curvature) HIPCHK(d_curv.alloc(nt));
    if ((rc = knn_launch<true>(c, tree, k, neighbor_r2(c), nullptr, nullptr, ko, d_n, d_curv.p))) return rc;
    if (out_normals) HIPCHK(hipMemcpyAsync(out_normals, d_n, sizeof(float) * 3 * nt, hipMemcpyDeviceToHost, c->stream));
    if (out_curvature) HIPCHK(hipMemcpyAsync(out_curvature, d_curv.p, sizeof(float) * nt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return OA_OK;
}

// ================================================================================================
// stray points of a point-cloud target: fixed-radius counts, mean k-nearest distances, removal (EXTENSION; oa_outlier.hpp)
// ================================================================================================
namespace {
int radius_count_launch(oa_ctx *c, const KnnTree &t, double radius, int cap, int32_t *d_count)
{
    const float rf = (float)radius, r2 = rf * rf;
    const int wpb = oa::KNN_WPB;
    const unsigned blocks = wave_blocks(c, t.bp.cnt[1], wpb);
    if (cap > 0) hipLaunchKernelGGL((oa::k_bvh_radius_count<true>), dim3(blocks), dim3(64 * wpb), 0, c->stream, t.bp, t.box, t.prims, r2, cap, d_count);
    else hipLaunchKernelGGL((oa::k_bvh_radius_count<false>), dim3(blocks), dim3(64 * wpb), 0, c->stream, t.bp, t.box, t.prims, r2, 0, d_count);
    HIPCHK(hipGetLastError());
    return OA_OK;
}

int knn_score_launch(oa_ctx *c, const KnnTree &t, int k, double *d_score)
{
    const int k1 = k + 1, wpb = oa::KNN_WPB;
    hipLaunchKernelGGL(oa::k_bvh_knn_score, dim3(wave_blocks(c, t.bp.cnt[1], wpb)), dim3(64 * wpb), 0, c->stream, t.bp, t.box, t.prims, k1, d_score);
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// Mean, standard deviation and threshold = mean + std_ratio std of the finite entries of d_score (nt of them) into *d_st, which
// the caller has zeroed: two passes in a fixed order, per-workgroup rows and then one workgroup (oa_outlier.hpp).  The rows are
// this function's own (their release is ordered on the stream, behind the launches).
int score_mean_std(oa_ctx *c, const double *d_score, int nt, double std_ratio, oa::OutlierStats *d_st)
{
    const int rows = oa::outlier_rows((long long)nt);
    DevTmp<double> d_sum;
    DevTmp<long long> d_n;
    HIPCHK(d_sum.alloc((size_t)rows)); HIPCHK(d_n.alloc((size_t)rows));
    const dim3 grid((unsigned)rows), blk(oa::OUT_THREADS);
    hipLaunchKernelGGL((oa::k_outlier_rows<0>), grid, blk, 0, c->stream, d_score, (long long)nt, (const oa::OutlierStats *)d_st, d_sum.p, d_n.p);
    hipLaunchKernelGGL((oa::k_outlier_finish<0>), dim3(1), blk, 0, c->stream, (const double *)d_sum.p, (const long long *)d_n.p, rows, std_ratio, d_st);
    hipLaunchKernelGGL((oa::k_outlier_rows<1>), grid, blk, 0, c->stream, d_score, (long long)nt, (const oa::OutlierStats *)d_st, d_sum.p, d_n.p);
    hipLaunchKernelGGL((oa::k_outlier_finish<1>), dim3(1), blk, 0, c->stream, (const double *)d_sum.p, (const long long *)d_n.p, rows, std_ratio, d_st);
    HIPCHK(hipGetLastError());
    return OA_OK;
}

// What a keep mask leaves of a cloud target (oa_target_outliers, oa_target_clusters): the flags' scan, the kept vertices' indices
// in ascending order and, to apply, their coordinates.
struct KeptVertices {
    DevTmp<long long> d_off;
    DevTmp<int32_t> d_index;
    DevTmp<float> d_xyz;
    DevTmp<char> scan_tmp;

    int alloc(size_t nt, int apply)
    {
        HIPCHK(d_off.alloc(nt + 1)); HIPCHK(d_index.alloc(nt));
        if (apply) HIPCHK(d_xyz.alloc(3 * nt));
        return OA_OK;
    }

    // d_flag: one int per vertex, 1 = keep; d_st->n_kept = their number (nothing else of *d_st is written)
    int compact(oa_ctx *c, const int *d_flag, oa::OutlierStats *d_st)
    {
        const int nt = c->tgt.nt;
        if (const int rc = scan_counts(c, d_flag, nt, d_off.p, scan_tmp)) return rc;
        hipLaunchKernelGGL(oa::k_outlier_compact, dim3((unsigned)(((size_t)nt + oa::OUT_THREADS - 1) / oa::OUT_THREADS)), dim3(oa::OUT_THREADS), 0, c->stream, d_flag,
                           (const long long *)d_off.p, nt, (const float *)c->tgt.d_tgt_xyz, d_index.p, d_xyz.p, d_st);
        HIPCHK(hipGetLastError());
        return OA_OK;
    }

    // The caller has read n_kept back and checked it: keep and kept_index go out (each may be null), the stream is waited for.
    // apply: the kept vertices become the target, as an upload from device memory would make them (the tree of this call goes
    // with the old target); with nothing kept the call is refused and the target stays.
    int finish(oa_ctx *c, const char *who, long long n_kept, int apply, const unsigned char *d_keep, uint8_t *keep, int32_t *kept_index)
    {
        const int nt = c->tgt.nt;
        if (keep) HIPCHK(hipMemcpyAsync(keep, d_keep, (size_t)nt, hipMemcpyDeviceToHost, c->stream));
        if (kept_index && n_kept > 0) HIPCHK(hipMemcpyAsync(kept_index, d_index.p, sizeof(int32_t) * (size_t)n_kept, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (!apply) return OA_OK;
        if (n_kept < 1) return fail(OA_E_TOO_FEW_PAIRS, "%s: no vertex of %d would be kept; the target stays as it is", who, nt);
        if (const int rc = set_target_common(c, d_xyz.p, (int64_t)n_kept, 1, true)) return rc;
        c->tgt.cleaned = (long long)nt - n_kept;
        return OA_OK;
    }
};
}  // namespace

OA_EXPORT int oa_target_radius_count(oa_ctx *c, double radius, int32_t cap, int32_t *count)
{
    static const char who[] = "oa_target_radius_count";
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    OA_NOT_MULTI(c, "oa_target_radius_count");
    if (!(radius > 0.0) || !(radius < (double)INFINITY)) return fail(OA_E_BAD_ARG, "%s: radius = %g (finite and > 0)", who, radius);
    if (cap < 0) return fail(OA_E_BAD_ARG, "%s: cap = %d (>= 0; 0: no cap)", who, (int)cap);
    int rc = cloud_call_begin(c, who, CloudCall::STRAYS);
    if (rc) return rc;
    KnnTree tree;
    if ((rc = knn_tree(c, tree))) return rc;
    const size_t nt = (size_t)c->tgt.nt;
    DevTmp<int32_t> d_count;
    HIPCHK(d_count.alloc(nt));
    if ((rc = radius_count_launch(c, tree, radius, cap, d_count.p))) return rc;
    if (count) HIPCHK(hipMemcpyAsync(count, d_count.p, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return OA_OK;
}

// ================================================================================================
// radius-limited neighbourhoods and the cloud's own point spacing (EXTENSION; oa_knn.hpp)
// ================================================================================================
OA_EXPORT int oa_set_neighbor_radius(oa_ctx *c, float radius)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    // 0 (either sign): off.  Else finite, > 0, and its float32 square finite -- the constant the searches compare against
    if (!(radius >= 0.f) || !(radius < INFINITY) || !(radius * radius < INFINITY))
        return fail(OA_E_BAD_ARG, "oa_set_neighbor_radius: radius = %g (0: no limit; else finite, > 0, and its float32 square finite)", (double)radius);
    if (radius == 0.f) radius = 0.f;                                 // (-0 reads back as 0)
    if (radius != c->nbr_radius) {
        if (const int rc = end_sequence(c)) return rc;
        c->nbr_radius = radius;
    }
    OA_ROUTE_ALL(c, oa_set_neighbor_radius(sub, radius));
    return OA_OK;
}

OA_EXPORT int oa_get_neighbor_radius(oa_ctx *c, float *radius)
{
    if (!c || !radius) return fail(OA_E_BAD_ARG, "oa_get_neighbor_radius: null argument");
    *radius = c->nbr_radius;
    return OA_OK;
}

OA_EXPORT int oa_target_spacing(oa_ctx *c, oa_spacing_report *rep)
{
    static const char who[] = "oa_target_spacing";
    if (!c || !rep) return fail(OA_E_BAD_ARG, "%s: null argument", who);
    OA_NOT_MULTI(c, "oa_target_spacing");
    memset(rep, 0, sizeof *rep);
    int rc = cloud_call_begin(c, who, CloudCall::STRAYS);
    if (rc) return rc;
    const int nt = c->tgt.nt;
    KnnTree tree;
    if ((rc = knn_tree(c, tree))) return rc;
    // the distance to the nearest other vertex = the statistical filter's score at k = 1; its mean and standard deviation by that
    // filter's fixed-order passes
    DevTmp<double> d_score;
    DevTmp<oa::OutlierStats> d_st;
    HIPCHK(d_score.alloc((size_t)nt)); HIPCHK(d_st.alloc(1));
    HIPCHK(hipMemsetAsync(d_st.p, 0, sizeof(oa::OutlierStats), c->stream));
    if ((rc = knn_score_launch(c, tree, 1, d_score.p))) return rc;
    if ((rc = score_mean_std(c, d_score.p, nt, 0.0, d_st.p))) return rc;
    oa::OutlierStats st;
    if ((rc = read_small(c, &st, d_st.p, sizeof st))) return rc;   // (waits for everything above)
    if (st.n_finite < 0 || st.n_finite > nt) return fail(OA_E_HIP, "%s: %lld of %d vertices with a spacing (internal)", who, st.n_finite, nt);
    rep->mean = st.mean; rep->std = st.std;
    rep->n_finite = (int64_t)st.n_finite; rep->n_nonfinite = (int64_t)nt - (int64_t)st.n_finite;
    return OA_OK;
}

OA_EXPORT int oa_target_outliers(oa_ctx *c, const oa_outlier_settings *s, int apply, uint8_t *keep, double *score, int32_t *count,
                                 int32_t *kept_index, oa_outlier_report *rep)
{
    static const char who[] = "oa_target_outliers";
    if (!c || !s) return fail(OA_E_BAD_ARG, "%s: null argument", who);
    OA_NOT_MULTI(c, "oa_target_outliers");
    if (rep) memset(rep, 0, sizeof *rep);
    const bool statistical = s->method == OA_OUTLIER_STATISTICAL;
    if (!statistical && s->method != OA_OUTLIER_RADIUS)
        return fail(OA_E_BAD_ARG, "%s: method %d (use OA_OUTLIER_STATISTICAL / OA_OUTLIER_RADIUS)", who, (int)s->method);
    if (statistical) {
        if (s->k < 1 || s->k > oa::KNN_MAX_K - 1) return fail(OA_E_BAD_ARG, "%s: k = %d outside 1 .. %d", who, (int)s->k, oa::KNN_MAX_K - 1);
        if (!(s->std_ratio >= 0.0) || !(s->std_ratio < (double)INFINITY)) return fail(OA_E_BAD_ARG, "%s: std_ratio = %g (finite and >= 0)", who, s->std_ratio);
    } else {
        if (!(s->radius > 0.0) || !(s->radius < (double)INFINITY)) return fail(OA_E_BAD_ARG, "%s: radius = %g (finite and > 0)", who, s->radius);
        if (s->min_neighbors < 1) return fail(OA_E_BAD_ARG, "%s: min_neighbors = %d (>= 1)", who, (int)s->min_neighbors);
        if (s->count_cap != 0 && (long long)s->count_cap < (long long)s->min_neighbors + 1)
            return fail(OA_E_BAD_ARG, "%s: count_cap = %d (0: exact counts, or >= min_neighbors + 1 = %lld)", who, (int)s->count_cap, (long long)s->min_neighbors + 1);
    }
    int rc = cloud_call_begin(c, who, CloudCall::STRAYS);
    if (rc) return rc;
    const int nt = c->tgt.nt;
    if (statistical && s->k > nt - 1) return fail(OA_E_BAD_ARG, "%s: k = %d outside 1 .. min(%d, %d target vertices - 1)", who, (int)s->k, oa::KNN_MAX_K - 1, nt);
    KnnTree tree;
    if ((rc = knn_tree(c, tree))) return rc;
    const size_t snt = (size_t)nt;
    const float *d_xyz = c->tgt.d_tgt_xyz;
    // 1. the per-vertex figure
    DevTmp<double> d_score;
    DevTmp<int32_t> d_count;
    DevTmp<oa::OutlierStats> d_st;
    HIPCHK(d_st.alloc(1));
    HIPCHK(hipMemsetAsync(d_st.p, 0, sizeof(oa::OutlierStats), c->stream));
    if (statistical) {
        HIPCHK(d_score.alloc(snt));
        if ((rc = knn_score_launch(c, tree, s->k, d_score.p))) return rc;
        // 2. mean, standard deviation and threshold of the finite scores
        if ((rc = score_mean_std(c, d_score.p, nt, s->std_ratio, d_st.p))) return rc;
    } else {
        HIPCHK(d_count.alloc(snt));
        if ((rc = radius_count_launch(c, tree, s->radius, s->count_cap, d_count.p))) return rc;
    }
    // 3. flags, their scan, the kept vertices in ascending order (and, to apply, their coordinates)
    DevTmp<int> d_flag;
    DevTmp<unsigned char> d_keep;
    KeptVertices kept;
    HIPCHK(d_flag.alloc(snt)); HIPCHK(d_keep.alloc(snt));
    if ((rc = kept.alloc(snt, apply))) return rc;
    const unsigned v_blocks = (unsigned)((snt + oa::OUT_THREADS - 1) / oa::OUT_THREADS);
    hipLaunchKernelGGL(oa::k_outlier_flags, dim3(v_blocks), dim3(oa::OUT_THREADS), 0, c->stream, statistical ? oa::OUT_STATISTICAL : oa::OUT_RADIUS, (const double *)d_score.p,
                       (const int32_t *)d_count.p, d_xyz, nt, (int)s->min_neighbors, d_st.p, d_flag.p, d_keep.p);
    HIPCHK(hipGetLastError());
    if ((rc = kept.compact(c, d_flag.p, d_st.p))) return rc;
    oa::OutlierStats st;
    if ((rc = read_small(c, &st, d_st.p, sizeof st))) return rc;   // (waits for everything above)
    if (st.n_kept < 0 || st.n_kept > nt) return fail(OA_E_HIP, "%s: %lld of %d vertices kept (internal)", who, st.n_kept, nt);
    if (score && statistical) HIPCHK(hipMemcpyAsync(score, d_score.p, sizeof(double) * snt, hipMemcpyDeviceToHost, c->stream));
    if (count && !statistical) HIPCHK(hipMemcpyAsync(count, d_count.p, sizeof(int32_t) * snt, hipMemcpyDeviceToHost, c->stream));
    if (rep) {
        rep->n_kept = (int64_t)st.n_kept; rep->n_removed = (int64_t)nt - (int64_t)st.n_kept; rep->n_nonfinite = (int64_t)st.n_nonfinite;
        if (statistical) { rep->mean = st.mean; rep->std = st.std; rep->threshold = st.threshold; }
    }
    // 4. keep and kept_index go out; to apply, the kept vertices become the target
    return kept.finish(c, who, st.n_kept, apply, d_keep.p, keep, kept_index);
}

// ================================================================================================
// the parts of a point-cloud target: DBSCAN labels, sizes, the largest part (EXTENSION; oa_cluster.hpp)
// ================================================================================================
OA_EXPORT int oa_target_clusters(oa_ctx *c, const oa_cluster_settings *s, int apply, int32_t *label, int32_t *sizes, uint8_t *keep,
                                 int32_t *kept_index, oa_cluster_report *rep)
{
    static const char who[] = "oa_target_clusters";
    if (!c || !s) return fail(OA_E_BAD_ARG, "%s: null argument", who);
    OA_NOT_MULTI(c, "oa_target_clusters");
    if (rep) memset(rep, 0, sizeof *rep);
    if (!(s->eps > 0.0) || !(s->eps < (double)INFINITY)) return fail(OA_E_BAD_ARG, "%s: eps = %g (finite and > 0)", who, s->eps);
    if (s->min_points < 1) return fail(OA_E_BAD_ARG, "%s: min_points = %d (>= 1)", who, (int)s->min_points);
    if (s->keep != OA_CLUSTER_KEEP_CLUSTERED && s->keep != OA_CLUSTER_KEEP_LARGEST && s->keep != OA_CLUSTER_KEEP_MIN_SIZE)
        return fail(OA_E_BAD_ARG, "%s: keep = %d (use OA_CLUSTER_KEEP_CLUSTERED / _LARGEST / _MIN_SIZE)", who, (int)s->keep);
    if (s->min_size < 0) return fail(OA_E_BAD_ARG, "%s: min_size = %lld (>= 0)", who, (long long)s->min_size);
    int rc = cloud_call_begin(c, who, CloudCall::STRAYS);
    if (rc) return rc;
    const int nt = c->tgt.nt;
    KnnTree tree;
    if ((rc = knn_tree(c, tree))) return rc;
    const size_t snt = (size_t)nt;
    const float *d_xyz = c->tgt.d_tgt_xyz;
    const float ef = (float)s->eps, r2 = ef * ef;
    const int min_points = (int)s->min_points;
    DevTmp<int32_t> d_count, d_label, d_sizes;
    DevTmp<uint32_t> d_parent, d_root, d_border;
    DevTmp<int> d_is_root, d_flag;
    DevTmp<long long> d_dense;
    DevTmp<unsigned char> d_keep;
    KeptVertices kept;
    DevTmp<oa::ClusterStats> d_st;
    DevTmp<oa::OutlierStats> d_ost;                                  // (the number kept)
    DevTmp<char> scan_tmp;
    HIPCHK(d_count.alloc(snt)); HIPCHK(d_label.alloc(snt)); HIPCHK(d_sizes.alloc(snt));
    HIPCHK(d_parent.alloc(snt)); HIPCHK(d_root.alloc(snt)); HIPCHK(d_border.alloc(snt));
    HIPCHK(d_is_root.alloc(snt)); HIPCHK(d_flag.alloc(snt)); HIPCHK(d_dense.alloc(snt + 1));
    HIPCHK(d_keep.alloc(snt)); HIPCHK(d_st.alloc(1)); HIPCHK(d_ost.alloc(1));
    if ((rc = kept.alloc(snt, apply))) return rc;
    HIPCHK(hipMemsetAsync(d_st.p, 0, sizeof(oa::ClusterStats), c->stream));
    HIPCHK(hipMemsetAsync(d_ost.p, 0, sizeof(oa::OutlierStats), c->stream));
    HIPCHK(hipMemsetAsync(d_sizes.p, 0, sizeof(int32_t) * snt, c->stream));
    HIPCHK(hipMemsetAsync(d_border.p, 0xff, sizeof(uint32_t) * snt, c->stream));
    // 1. core flags: counts that saturate at min_points
    if ((rc = radius_count_launch(c, tree, s->eps, min_points, d_count.p))) return rc;
    // 2. the core graph's components (link, then flatten in a launch of its own), 3. the border vertices' lowest root
    const int wpb = oa::KNN_WPB;
    const unsigned t_blocks = wave_blocks(c, tree.bp.cnt[1], wpb);
    const unsigned v_blocks = (unsigned)((snt + oa::CL_THREADS - 1) / oa::CL_THREADS);
    const int max_steps = (int)std::min<long long>(2ll * nt + 64, 0x7fffffffll);
    const dim3 blk(oa::CL_THREADS);
    hipLaunchKernelGGL(oa::k_cluster_init, dim3(v_blocks), blk, 0, c->stream, nt, d_parent.p);
    hipLaunchKernelGGL((oa::k_bvh_cluster<oa::CL_LINK>), dim3(t_blocks), dim3(64 * wpb), 0, c->stream, tree.bp, tree.box, tree.prims, r2, min_points,
                       (const int32_t *)d_count.p, d_parent.p, (const uint32_t *)nullptr, (uint32_t *)nullptr, max_steps, d_st.p);
    hipLaunchKernelGGL(oa::k_cluster_flatten, dim3(v_blocks), blk, 0, c->stream, (const uint32_t *)d_parent.p, (const int32_t *)d_count.p, min_points, nt, d_root.p,
                       d_is_root.p, d_st.p);
    hipLaunchKernelGGL((oa::k_bvh_cluster<oa::CL_BORDER>), dim3(t_blocks), dim3(64 * wpb), 0, c->stream, tree.bp, tree.box, tree.prims, r2, min_points,
                       (const int32_t *)d_count.p, (uint32_t *)nullptr, (const uint32_t *)d_root.p, d_border.p, max_steps, d_st.p);
    HIPCHK(hipGetLastError());
    // 4. dense labels in ascending root order, sizes, the largest cluster, the keep flags and their compaction
    if ((rc = scan_counts(c, d_is_root.p, nt, d_dense.p, scan_tmp))) return rc;
    hipLaunchKernelGGL(oa::k_cluster_label, dim3(v_blocks), blk, 0, c->stream, (const uint32_t *)d_root.p, (const uint32_t *)d_border.p, (const long long *)d_dense.p,
                       d_xyz, nt, d_label.p, d_sizes.p, d_st.p);
    hipLaunchKernelGGL(oa::k_cluster_largest, dim3(1), blk, 0, c->stream, (const int32_t *)d_sizes.p, d_st.p);
    hipLaunchKernelGGL(oa::k_cluster_keep, dim3(v_blocks), blk, 0, c->stream, (const int32_t *)d_label.p, (const int32_t *)d_sizes.p, (const oa::ClusterStats *)d_st.p,
                       (int)s->keep, (long long)s->min_size, nt, d_flag.p, d_keep.p);
    HIPCHK(hipGetLastError());
    if ((rc = kept.compact(c, d_flag.p, d_ost.p))) return rc;
    oa::ClusterStats st;
    oa::OutlierStats ost;
    if ((rc = read_small(c, &st, d_st.p, sizeof st))) return rc;    // (waits for everything above)
    if ((rc = read_small(c, &ost, d_ost.p, sizeof ost))) return rc;
    if (st.err) return fail(OA_E_HIP, "%s: the union-find ran out of its %d steps (flag %d; internal)", who, max_steps, st.err);
    if (ost.n_kept < 0 || ost.n_kept > nt || st.n_clusters < 0 || st.n_clusters > nt)
        return fail(OA_E_HIP, "%s: %lld of %d vertices kept in %lld clusters (internal)", who, ost.n_kept, nt, st.n_clusters);
    if (label) HIPCHK(hipMemcpyAsync(label, d_label.p, sizeof(int32_t) * snt, hipMemcpyDeviceToHost, c->stream));
    if (sizes && st.n_clusters > 0) HIPCHK(hipMemcpyAsync(sizes, d_sizes.p, sizeof(int32_t) * (size_t)st.n_clusters, hipMemcpyDeviceToHost, c->stream));
    if (rep) {
        rep->n_clusters = (int64_t)st.n_clusters; rep->n_core = (int64_t)st.n_core; rep->n_border = (int64_t)st.n_border;
        rep->n_noise = (int64_t)st.n_noise; rep->n_nonfinite = (int64_t)st.n_nonfinite;
        rep->largest_label = (int64_t)st.largest_label; rep->largest_size = (int64_t)st.largest_size;
        rep->n_kept = (int64_t)ost.n_kept; rep->n_removed = (int64_t)nt - (int64_t)ost.n_kept;
    }
    // 5. keep and kept_index go out; to apply, the kept vertices become the target
    return kept.finish(c, who, ost.n_kept, apply, d_keep.p, keep, kept_index);
}

// ================================================================================================
// one consistent sign for a cloud's normals: a minimum spanning forest of the neighbour graph (EXTENSION; oa_orient.hpp)
// ================================================================================================
OA_EXPORT int oa_orient_target_normals(oa_ctx *c, int k, double max_dist, int seed, const float point[3], const float *normals, int install,
                                       float *out_normals, uint8_t *out_flipped, int32_t *out_component, oa_orient_report *rep)
{
    static const char who[] = "oa_orient_target_normals";
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    OA_NOT_MULTI(c, "oa_orient_target_normals");
    if (rep) memset(rep, 0, sizeof *rep);
    if (seed != OA_SEED_KEEP && seed != OA_SEED_TOWARD && seed != OA_SEED_AWAY)
        return fail(OA_E_BAD_ARG, "%s: seed %d (use OA_SEED_KEEP / OA_SEED_TOWARD / OA_SEED_AWAY)", who, seed);
    if (seed == OA_SEED_TOWARD && !point) return fail(OA_E_BAD_ARG, "%s: OA_SEED_TOWARD needs a point", who);
    if (point)
        for (int a = 0; a < 3; ++a)
            if (!(fabsf(point[a]) < INFINITY)) return fail(OA_E_BAD_ARG, "%s: point[%d] = %g is not finite", who, a, (double)point[a]);
    if (!(max_dist >= 0.0) || !(max_dist < (double)INFINITY)) return fail(OA_E_BAD_ARG, "%s: max_dist = %g (finite and >= 0; 0: no cap)", who, max_dist);
    int rc = cloud_call_begin(c, who, CloudCall::NEIGHBOURS, k, 2);
    if (rc) return rc;
    if (!normals && !c->tgt.d_tgt_n)
        return fail(OA_E_STATE, "%s: no normals given and the target has none (oa_set_target_normals, oa_set_normals or oa_estimate_target_normals with install)", who);
    const int nt = c->tgt.nt;
    const long long n_ent = (long long)nt * k;
    if (n_ent > oa::SORT_MAX_N) return fail(OA_E_CAPACITY, "%s: %d vertices x k = %d is %lld entries (at most 2^31 - 2^20)", who, nt, k, n_ent);
    oa::OrientSeed sd{};
    sd.mode = seed;
    if (seed != OA_SEED_KEEP && (rc = orient_point_or_centroid(c, who, point, sd.p))) return rc;
    const size_t snt = (size_t)nt, sne = (size_t)n_ent;
    const float *d_xyz = c->tgt.d_tgt_xyz;
    DevTmp<float> tmp_in;
    const float *d_nrm = c->tgt.d_tgt_n;
    if (normals && (rc = stage_floats(c, normals, 3 * snt, 0, tmp_in, d_nrm))) return rc;
    // 1. the rows of oa_target_knn(k)
    KnnTree tree;
    if ((rc = knn_tree(c, tree))) return rc;
    DevTmp<int32_t> d_idx;
    DevTmp<float> d_d2;
    HIPCHK(d_idx.alloc(sne)); HIPCHK(d_d2.alloc(sne));
    if ((rc = knn_launch<false>(c, tree, k, INFINITY, d_idx.p, d_d2.p, oa::KnnOrient{}, nullptr, nullptr))) return rc;
    // 2. the entries that are edges, their keys, and their places in the order (w, lo, hi): three stable passes, the last key first
    const unsigned v_blocks = (unsigned)((snt + oa::ORI_THREADS - 1) / oa::ORI_THREADS), e_blocks = (unsigned)((sne + oa::ORI_THREADS - 1) / oa::ORI_THREADS);
    const dim3 blk(oa::ORI_THREADS);
    DevTmp<uint8_t> d_elig, d_cflip;
    DevTmp<uint32_t> d_P, d_Q, d_best, d_ent, d_kw, d_klo, d_khi;
    DevTmp<int> d_ord, d_ord2;
    DevTmp<oa::OrientRound> d_round;
    HIPCHK(d_elig.alloc(snt)); HIPCHK(d_cflip.alloc(snt)); HIPCHK(d_P.alloc(snt)); HIPCHK(d_Q.alloc(snt)); HIPCHK(d_best.alloc(snt));
    HIPCHK(d_ent.alloc(sne)); HIPCHK(d_kw.alloc(sne)); HIPCHK(d_klo.alloc(sne)); HIPCHK(d_khi.alloc(sne));
    HIPCHK(d_ord.alloc(sne)); HIPCHK(d_ord2.alloc(sne)); HIPCHK(d_round.alloc(1));
    const float md = (float)max_dist, cap2 = md * md;
    hipLaunchKernelGGL(oa::k_orient_init, dim3(v_blocks), blk, 0, c->stream, d_xyz, d_nrm, nt, d_elig.p, d_P.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(oa::k_orient_entries, dim3(e_blocks), blk, 0, c->stream, (const int32_t *)d_idx.p, (const float *)d_d2.p, d_nrm, (const uint8_t *)d_elig.p, nt, k,
                       n_ent, max_dist > 0.0 ? 1 : 0, cap2, d_ent.p, d_kw.p, d_klo.p, d_khi.p);
    HIPCHK(hipGetLastError());
    const int idx_bits = bits_for((long long)nt);
    if ((rc = sort_order_bits(c, d_khi.p, d_ord.p, sne, idx_bits))) return rc;
    if ((rc = lex_order_next(c, d_klo.p, idx_bits, d_ord.p, d_ord2.p, sne))) return rc;
    if ((rc = lex_order_next(c, d_kw.p, oa::ORI_W_BITS, d_ord2.p, d_ord.p, sne))) return rc;
    uint32_t *const d_rank = d_khi.p;                               // (the keys have been read)
    hipLaunchKernelGGL(oa::k_orient_rank, dim3(e_blocks), blk, 0, c->stream, (const int *)d_ord.p, n_ent, d_rank);
    HIPCHK(hipGetLastError());
    // 3. Boruvka rounds.  Every round with a hook at least halves the components that still have an edge out, and one round more
    //    finds none: at most ceil(log2 nt) + 1.  After the hooks nobody stands deeper than `roots` below a root, a jump halves
    //    the depth and one jump more changes nothing: at most ceil(log2 roots) + 1 jumps.  One read per round.
    const int max_rounds = bits_for((long long)nt) + 1;
    long long roots = nt;
    int rounds = 0;
    bool done = false;
    for (int r = 0; r < max_rounds && !done; ++r) {
        HIPCHK(hipMemsetAsync(d_best.p, 0xff, sizeof(uint32_t) * snt, c->stream));
        HIPCHK(hipMemsetAsync(d_round.p, 0, sizeof(oa::OrientRound), c->stream));
        hipLaunchKernelGGL(oa::k_orient_min, dim3(e_blocks), blk, 0, c->stream, (const uint32_t *)d_ent.p, (const uint32_t *)d_rank, (const uint32_t *)d_P.p, k, n_ent,
                           d_best.p);
        hipLaunchKernelGGL(oa::k_orient_hook, dim3(v_blocks), blk, 0, c->stream, (const uint32_t *)d_P.p, (const uint32_t *)d_best.p, (const int *)d_ord.p,
                           (const uint32_t *)d_ent.p, nt, k, n_ent, d_Q.p, d_round.p);
        const int jumps = std::min(oa::ORI_MAX_JUMPS, bits_for(std::max(roots, 2ll)) + 1);
        for (int j = 1; j <= jumps; ++j)
            hipLaunchKernelGGL(oa::k_orient_jump, dim3(v_blocks), blk, 0, c->stream, (const uint32_t *)((j & 1) ? d_Q.p : d_P.p), (j & 1) ? d_P.p : d_Q.p, nt, j, d_round.p);
        HIPCHK(hipGetLastError());
        oa::OrientRound h;
        if ((rc = read_small(c, &h, d_round.p, sizeof h))) return rc;
        if (h.changed[jumps]) return fail(OA_E_HIP, "%s: round %d did not settle in %d pointer jumps (internal)", who, r + 1, jumps);
        if (h.hooked < 0 || h.hooked >= roots) return fail(OA_E_HIP, "%s: round %d hooked %d of %lld roots (internal)", who, r + 1, h.hooked, roots);
        if (h.hooked == 0) done = true;
        else { ++rounds; roots -= h.hooked; }
    }
    if (!done) return fail(OA_E_HIP, "%s: components still merging after %d rounds (internal)", who, max_rounds);
    // 4. labels, seeds, every component's sign, the normals
    DevTmp<unsigned long long> d_dkey;
    DevTmp<uint32_t> d_seed_of;
    DevTmp<oa::OrientInfo> d_info;
    DevTmp<float> tmp_out;
    DevTmp<uint8_t> d_flipped;
    DevTmp<int32_t> d_comp;
    HIPCHK(d_info.alloc(1));
    if (out_flipped) HIPCHK(d_flipped.alloc(snt));
    if (out_component) HIPCHK(d_comp.alloc(snt));
    uint32_t *const d_label = d_best.p;
    HIPCHK(hipMemsetAsync(d_label, 0xff, sizeof(uint32_t) * snt, c->stream));
    HIPCHK(hipMemsetAsync(d_info.p, 0, sizeof(oa::OrientInfo), c->stream));
    if (seed != OA_SEED_KEEP) {
        HIPCHK(d_dkey.alloc(snt)); HIPCHK(d_seed_of.alloc(snt));
        HIPCHK(hipMemsetAsync(d_dkey.p, seed == OA_SEED_TOWARD ? 0xff : 0, sizeof(unsigned long long) * snt, c->stream));
        HIPCHK(hipMemsetAsync(d_seed_of.p, 0xff, sizeof(uint32_t) * snt, c->stream));
    }
    hipLaunchKernelGGL(oa::k_orient_label, dim3(v_blocks), blk, 0, c->stream, (const uint32_t *)d_P.p, (const uint8_t *)d_elig.p, d_xyz, nt, sd, d_label, d_dkey.p);
    if (seed != OA_SEED_KEEP)
        hipLaunchKernelGGL(oa::k_orient_seed, dim3(v_blocks), blk, 0, c->stream, (const uint32_t *)d_P.p, (const uint8_t *)d_elig.p, d_xyz, nt, sd,
                           (const unsigned long long *)d_dkey.p, d_seed_of.p);
    hipLaunchKernelGGL(oa::k_orient_sign, dim3(v_blocks), blk, 0, c->stream, (const uint32_t *)d_P.p, (const uint8_t *)d_elig.p, d_xyz, d_nrm, nt, sd,
                       (const uint32_t *)(seed != OA_SEED_KEEP ? d_seed_of.p : d_label), d_cflip.p, d_info.p);
    HIPCHK(hipGetLastError());
    float *d_out = nullptr;
    if ((rc = new_normals_dest(c, install, out_normals != nullptr, tmp_out, d_out))) return rc;
    hipLaunchKernelGGL(oa::k_orient_apply, dim3(v_blocks), blk, 0, c->stream, (const uint32_t *)d_P.p, (const uint8_t *)d_elig.p, (const uint8_t *)d_cflip.p,
                       (const uint32_t *)d_label, d_nrm, nt, d_out, d_flipped.p, d_comp.p, d_info.p);
    HIPCHK(hipGetLastError());
    oa::OrientInfo info;
    if ((rc = read_small(c, &info, d_info.p, sizeof info))) return rc;
    if (out_normals) HIPCHK(hipMemcpyAsync(out_normals, d_out, sizeof(float) * 3 * snt, hipMemcpyDeviceToHost, c->stream));
    if (out_flipped) HIPCHK(hipMemcpyAsync(out_flipped, d_flipped.p, snt, hipMemcpyDeviceToHost, c->stream));
    if (out_component) HIPCHK(hipMemcpyAsync(out_component, d_comp.p, sizeof(int32_t) * snt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (rep) {
        rep->n_components = (int64_t)info.n_components; rep->n_left_out = (int64_t)info.n_left_out; rep->n_flipped = (int64_t)info.n_flipped;
        rep->rounds = rounds; rep->reserved = 0;
    }
    return OA_OK;
}

// ================================================================================================
// coarse alignment from matched descriptors (EXTENSION; oa_feat.hpp)
// ================================================================================================
namespace {
bool row_is_zero(const float *row, int dim)
{
    for (int k = 0; k < dim; ++k) if (row[k] != 0.0f) return false;
    return true;
}

// nearest and second nearest row of fb for every row of fa (host arrays in, host arrays out; any of the outputs may be null)
int match_rows(oa_ctx *c, const float *fa, int na, const float *fb, int nb, int dim, int32_t *out_idx, float *out_d2, float *out_second)
{
    const int DP = oa::feat_padded_dim(dim);
    const int na_pad = (na + oa::FEAT_QPB - 1) / oa::FEAT_QPB * oa::FEAT_QPB, nb_pad = (nb + oa::FEAT_TB - 1) / oa::FEAT_TB * oa::FEAT_TB;
    std::vector<float> ha((size_t)na_pad * DP, 0.0f), hb((size_t)nb_pad * DP, 0.0f), pen((size_t)nb_pad, INFINITY);
    for (int i = 0; i < na; ++i) memcpy(&ha[(size_t)i * DP], fa + (size_t)i * dim, sizeof(float) * (size_t)dim);
    for (int j = 0; j < nb; ++j) {
        memcpy(&hb[(size_t)j * DP], fb + (size_t)j * dim, sizeof(float) * (size_t)dim);
        if (!row_is_zero(fb + (size_t)j * dim, dim)) pen[(size_t)j] = 0.0f;
    }
    const int qblocks = na_pad / oa::FEAT_QPB, tiles = nb_pad / oa::FEAT_TB;
    int splits = std::max(1, std::min(std::min(tiles, oa::FEAT_MAX_SPLITS), (c->n_cu * 4 + qblocks - 1) / qblocks));
    const int tps = (tiles + splits - 1) / splits;
    splits = (tiles + tps - 1) / tps;                               // every split has a tile
    DevTmp<float> d_a, d_b, d_pen, d_psec, d_d2, d_sec;
    DevTmp<unsigned long long> d_keys, d_pkey;
    DevTmp<int32_t> d_idx;
    HIPCHK(d_a.alloc(ha.size())); HIPCHK(d_b.alloc(hb.size())); HIPCHK(d_pen.alloc(pen.size()));
    HIPCHK(d_keys.alloc((size_t)na_pad)); HIPCHK(d_pkey.alloc((size_t)splits * na_pad)); HIPCHK(d_psec.alloc((size_t)splits * na_pad));
    HIPCHK(d_idx.alloc((size_t)na)); HIPCHK(d_d2.alloc((size_t)na)); HIPCHK(d_sec.alloc((size_t)na));
    HIPCHK(hipMemcpyAsync(d_a.p, ha.data(), sizeof(float) * ha.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_b.p, hb.data(), sizeof(float) * hb.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_pen.p, pen.data(), sizeof(float) * pen.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(d_keys.p, 0xff, sizeof(unsigned long long) * (size_t)na_pad, c->stream));
    const dim3 grid((unsigned)qblocks, (unsigned)splits), block(oa::FEAT_THREADS);
    auto launch = [&](auto DPc) {
        hipLaunchKernelGGL((oa::k_match_features<decltype(DPc)::value>), grid, block, 0, c->stream, (const float *)d_a.p, (const float *)d_b.p,
                           (const float *)d_pen.p, na_pad, tiles, tps, d_keys.p, d_pkey.p, d_psec.p);
    };
    if (DP == 8) launch(std::integral_constant<int, 8>{});
    else if (DP == 16) launch(std::integral_constant<int, 16>{});
    else if (DP == 36) launch(std::integral_constant<int, 36>{});
    else launch(std::integral_constant<int, 64>{});
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(oa::k_match_finalize, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, c->stream, (const unsigned long long *)d_keys.p,
                       (const unsigned long long *)d_pkey.p, (const float *)d_psec.p, na, na_pad, splits, d_idx.p, d_d2.p, d_sec.p);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> h_idx((size_t)na);
    std::vector<float> h_d2((size_t)na), h_sec((size_t)na);
    HIPCHK(hipMemcpyAsync(h_idx.data(), d_idx.p, sizeof(int32_t) * (size_t)na, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(h_d2.data(), d_d2.p, sizeof(float) * (size_t)na, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(h_sec.data(), d_sec.p, sizeof(float) * (size_t)na, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < na; ++i) {
        const bool none = row_is_zero(fa + (size_t)i * dim, dim);   // a zero row does not query
        if (out_idx) out_idx[i] = none ? -1 : h_idx[(size_t)i];
        if (out_d2) out_d2[i] = none ? INFINITY : h_d2[(size_t)i];
        if (out_second) out_second[i] = none ? INFINITY : h_sec[(size_t)i];
    }
    return OA_OK;
}

int match_args(const char *who, const float *fa, int64_t na, const float *fb, int64_t nb, int dim)
{
    if (!fa || !fb) return fail(OA_E_BAD_ARG, "%s: null argument", who);
    if (dim < 1 || dim > oa::FEAT_MAX_DIM) return fail(OA_E_BAD_ARG, "%s: dim %d outside 1 .. %d", who, dim, oa::FEAT_MAX_DIM);
    if (na < 1 || nb < 1 || na > (1 << 24) || nb > (1 << 24)) return fail(OA_E_BAD_ARG, "%s: %lld and %lld rows (1 .. 2^24 each)", who, (long long)na, (long long)nb);
    return OA_OK;
}
}  // namespace

OA_EXPORT int oa_target_fpfh(oa_ctx *c, int k, float *out, int keep)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    OA_NOT_MULTI(c, "oa_target_fpfh");
    int rc = cloud_call_begin(c, "oa_target_fpfh", CloudCall::NEIGHBOURS, k, 4);
    if (rc) return rc;
    if (!c->tgt.d_tgt_n) return fail(OA_E_STATE, "oa_target_fpfh: the target has no normals (oa_set_target_normals, oa_set_normals or oa_estimate_target_normals with install)");
    KnnTree tree;
    if ((rc = knn_tree(c, tree))) return rc;
    const size_t nt = (size_t)c->tgt.nt;
    DevTmp<int32_t> d_idx;
    DevTmp<double> d_spfh;
    DevTmp<float> tmp;
    HIPCHK(d_idx.alloc(nt * (size_t)k));
    HIPCHK(d_spfh.alloc(nt * oa::FPFH_DIM));
    float *d_out = nullptr;
    if (keep) {                                                     // (the stream is idle: a kept table is replaced in place)
        if (!c->tgt.d_tgt_feat) HIPCHK(dev_malloc(&c->tgt.d_tgt_feat, sizeof(float) * oa::FPFH_DIM * nt));
        d_out = c->tgt.d_tgt_feat;
    } else { HIPCHK(tmp.alloc(oa::FPFH_DIM * nt)); d_out = tmp.p; }
    if ((rc = knn_launch<false>(c, tree, k, neighbor_r2(c), d_idx.p, nullptr, oa::KnnOrient{}, nullptr, nullptr))) return rc;
    const dim3 grid((unsigned)((nt + oa::FPFH_THREADS - 1) / oa::FPFH_THREADS)), block(oa::FPFH_THREADS);
    hipLaunchKernelGGL((oa::k_fpfh<false>), grid, block, 0, c->stream, (const float *)c->tgt.d_tgt_xyz, (const float *)c->tgt.d_tgt_n, (const int32_t *)d_idx.p,
                       c->tgt.nt, k, d_spfh.p, (float *)nullptr);
    hipLaunchKernelGGL((oa::k_fpfh<true>), grid, block, 0, c->stream, (const float *)c->tgt.d_tgt_xyz, (const float *)c->tgt.d_tgt_n, (const int32_t *)d_idx.p,
                       c->tgt.nt, k, d_spfh.p, d_out);
    HIPCHK(hipGetLastError());
    if (out) HIPCHK(hipMemcpyAsync(out, d_out, sizeof(float) * oa::FPFH_DIM * nt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return OA_OK;
}

OA_EXPORT int oa_match_features(oa_ctx *c, const float *fa, int64_t na, const float *fb, int64_t nb, int32_t dim, int32_t *out_idx, float *out_d2,
                                float *out_d2_second)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    OA_NOT_MULTI(c, "oa_match_features");
    int rc = match_args("oa_match_features", fa, na, fb, nb, dim);
    if (rc) return rc;
    if ((rc = use_device(c))) return rc;
    return match_rows(c, fa, (int)na, fb, (int)nb, dim, out_idx, out_d2, out_d2_second);
}

OA_EXPORT int oa_feature_candidates(oa_ctx *c, const float *src_feat, int64_t n_verts, const float *tgt_feat, const oa_feature_settings *fs,
                                    const int32_t *triples, float *mx_align_out, int32_t *n_out, oa_feature_report *rep)
{
    if (!c || !src_feat || !fs || !mx_align_out || !n_out || !rep) return fail(OA_E_BAD_ARG, "oa_feature_candidates: null argument");
    OA_NOT_MULTI(c, "oa_feature_candidates");
    int rc = pose_call_ready(c);
    if (rc) return rc;
    if (c->tgt.surface) return fail(OA_E_STATE, "oa_feature_candidates: a surface target (oa_set_target_mesh) has no per-vertex descriptors");
    if (!tgt_feat && !c->tgt.d_tgt_feat) return fail(OA_E_STATE, "oa_feature_candidates: no descriptors are resident for the target (oa_target_fpfh with keep), and none were passed");
    if (!tgt_feat && fs->dim != oa::FPFH_DIM) return fail(OA_E_BAD_ARG, "oa_feature_candidates: the resident descriptors have %d floats, the settings say %d", oa::FPFH_DIM, fs->dim);
    if (c->src.ns <= 0) return fail(OA_E_STATE, "oa_feature_candidates: the selection is empty");
    if (n_verts != c->src.src_n_verts) return fail(OA_E_BAD_ARG, "oa_feature_candidates: %lld descriptor rows for %lld source vertices", (long long)n_verts, c->src.src_n_verts);
    const int dim = fs->dim;
    if (dim < 1 || dim > oa::FEAT_MAX_DIM || fs->n_hyp < 1 || fs->n_hyp > 65535 || !(fs->ratio > 0.0) || !(fs->edge_tol > 0.0) || !(fs->edge_tol <= 1.0) ||
        !(fs->min_edge < INFINITY))
        return fail(OA_E_BAD_ARG, "oa_feature_candidates: dim 1 .. %d, n_hyp 1 .. 65535, ratio > 0, 0 < edge_tol <= 1 and a finite min_edge", oa::FEAT_MAX_DIM);
    if (c->src.ns > (1 << 24) || c->tgt.nt > (1 << 24)) return fail(OA_E_BAD_ARG, "oa_feature_candidates: more than 2^24 rows on a side");
    memset(rep, 0, sizeof *rep);
    *n_out = 0;
    const auto t0 = std::chrono::steady_clock::now();
    auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    const int ns = c->src.ns, nt = c->tgt.nt, n_hyp = fs->n_hyp;
    // the selection's rows, in slot order
    std::vector<int> sel((size_t)ns);
    HIPCHK(hipMemcpyAsync(sel.data(), c->src.d_sel, sizeof(int) * (size_t)ns, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<float> fsel((size_t)ns * dim);
    for (int s = 0; s < ns; ++s) {
        if (sel[(size_t)s] < 0 || sel[(size_t)s] >= n_verts) return fail(OA_E_STATE, "oa_feature_candidates: slot %d holds vertex %d of %lld", s, sel[(size_t)s], (long long)n_verts);
        memcpy(&fsel[(size_t)s * dim], src_feat + (size_t)sel[(size_t)s] * dim, sizeof(float) * (size_t)dim);
    }
    std::vector<float> kept;
    if (!tgt_feat) {                                                // the kept table (matching takes host rows)
        kept.resize((size_t)nt * oa::FPFH_DIM);
        HIPCHK(hipMemcpyAsync(kept.data(), c->tgt.d_tgt_feat, sizeof(float) * kept.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        tgt_feat = kept.data();
    }
    // 1. both directions
    std::vector<int32_t> st((size_t)ns), ts((size_t)nt);
    std::vector<float> st_d2((size_t)ns), st_sec((size_t)ns);
    const auto t1 = std::chrono::steady_clock::now();
    if ((rc = match_rows(c, fsel.data(), ns, tgt_feat, nt, dim, st.data(), st_d2.data(), st_sec.data()))) return rc;
    if (fs->mutual && (rc = match_rows(c, tgt_feat, nt, fsel.data(), ns, dim, ts.data(), nullptr, nullptr))) return rc;
    rep->match_ms = ms_since(t1);
    // 2., 3. the kept pairs
    std::vector<int> pair_s, pair_t;
    const double r2 = fs->ratio * fs->ratio;
    for (int s = 0; s < ns; ++s) {
        const int t = st[(size_t)s];
        if (t < 0) continue;
        if (!((double)st_d2[(size_t)s] <= r2 * (double)st_sec[(size_t)s])) continue;
        if (fs->mutual && ts[(size_t)t] != s) continue;
        pair_s.push_back(s); pair_t.push_back(t);
    }
    {   // by source vertex index: the slots are in the search's own order, the caller knows the vertices
        std::vector<int> order(pair_s.size());
        for (size_t k = 0; k < order.size(); ++k) order[k] = (int)k;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return sel[(size_t)pair_s[(size_t)a]] < sel[(size_t)pair_s[(size_t)b]]; });
        std::vector<int> ps(order.size()), pt(order.size());
        for (size_t k = 0; k < order.size(); ++k) { ps[k] = pair_s[(size_t)order[k]]; pt[k] = pair_t[(size_t)order[k]]; }
        pair_s.swap(ps); pair_t.swap(pt);
    }
    const int n_pairs = (int)pair_s.size();
    rep->n_pairs = n_pairs;
    if (n_pairs < 3) {                                              // 4. not an error
        rep->status = OA_FEAT_TOO_FEW_PAIRS;
        rep->total_ms = ms_since(t0);
        return OA_OK;
    }
    // 6. the triples
    std::vector<int32_t> tri(3 * (size_t)n_hyp);
    if (triples) memcpy(tri.data(), triples, sizeof(int32_t) * tri.size());
    else
        for (int h = 0; h < n_hyp; ++h)
            for (int k = 0; k < 3; ++k) tri[3 * (size_t)h + k] = (int32_t)oa::feat_hash_index(fs->seed, (uint32_t)h, (uint32_t)k, (uint32_t)n_pairs);
    double min_edge = fs->min_edge;
    if (!(min_edge > 0.0)) {                                        // 0.05 x the target's diagonal, in world units
        double lo[3], hi[3];
        if ((rc = target_bbox(c, lo, hi))) return rc;
        const float *B = c->h_state.mx2;
        double d2 = 0.0;
        for (int i = 0; i < 3; ++i) {
            double v = 0.0;
            for (int k = 0; k < 3; ++k) v += (double)B[4 * i + k] * (hi[k] - lo[k]);
            d2 += v * v;
        }
        min_edge = 0.05 * sqrt(d2);
    }
    // 7. one wave per hypothesis, then the accepted ones in order
    DevTmp<int> d_ps, d_pt, d_tri, d_flags, d_n;
    DevTmp<float> d_poses, d_out;
    HIPCHK(d_ps.alloc((size_t)n_pairs)); HIPCHK(d_pt.alloc((size_t)n_pairs)); HIPCHK(d_tri.alloc(tri.size()));
    HIPCHK(d_flags.alloc((size_t)n_hyp)); HIPCHK(d_n.alloc(1));
    HIPCHK(d_poses.alloc(16 * (size_t)n_hyp)); HIPCHK(d_out.alloc(16 * (size_t)n_hyp));
    HIPCHK(hipMemcpyAsync(d_ps.p, pair_s.data(), sizeof(int) * (size_t)n_pairs, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_pt.p, pair_t.data(), sizeof(int) * (size_t)n_pairs, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_tri.p, tri.data(), sizeof(int32_t) * tri.size(), hipMemcpyHostToDevice, c->stream));
    oa::Mat4f m1, m2;
    oa::Mat4d ma;
    memcpy(m1.m, c->h_state.mx1, sizeof m1.m);
    memcpy(m2.m, c->h_state.mx2, sizeof m2.m);
    for (int k = 0; k < 16; ++k) ma.m[k] = (double)c->h_state.mx1[k];
    constexpr int WPB = 4;
    hipLaunchKernelGGL((oa::k_triple_poses<WPB>), dim3((unsigned)((n_hyp + WPB - 1) / WPB)), dim3(WPB * 64), 0, c->stream, (const int *)d_ps.p,
                       (const int *)d_pt.p, n_pairs, (const int *)d_tri.p, n_hyp, (const float4 *)c->src.d_src4, (const float *)c->tgt.d_tgt_xyz, m1, m2, ma,
                       fs->edge_tol, min_edge, d_poses.p, d_flags.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(oa::k_triple_compact, dim3(1), dim3(256), 0, c->stream, (const float *)d_poses.p, (const int *)d_flags.p, n_hyp, d_out.p, d_n.p);
    HIPCHK(hipGetLastError());
    int n_acc = 0;
    if ((rc = read_small(c, &n_acc, d_n.p, sizeof n_acc))) return rc;
    if (n_acc < 0 || n_acc > n_hyp) return fail(OA_E_HIP, "oa_feature_candidates: %d poses out of %d hypotheses", n_acc, n_hyp);
    if (n_acc > 0 && (rc = read_small(c, mx_align_out, d_out.p, sizeof(float) * 16 * (size_t)n_acc))) return rc;
    *n_out = n_acc;
    rep->n_accepted = n_acc;
    rep->status = n_acc > 0 ? OA_OK : OA_FEAT_NO_POSE;
    rep->total_ms = ms_since(t0);
    return OA_OK;
}

// ================================================================================================
// voxel-grid downsampling (EXTENSION; oa_voxel.hpp)
// ================================================================================================
namespace {
// the cell of a coordinate, as k_voxel_keys computes it (the same three fp64 operations), kept a double: it may be huge
inline double voxel_cell_of(float x, double o, double h) { return floor(((double)x - o) / h); }

// order[0 .. n) = the stable ascending order of the keys' low `bits` bits (1 .. 64): one argsort for up to 32 bits, else the
// lexicographic order of their 30-bit slices, the lowest slice first
int voxel_sort_keys(oa_ctx *c, const unsigned long long *d_keys, int n, int bits, DevTmp<int> &order)
{
    const unsigned blocks = (unsigned)(((size_t)n + oa::VOX_THREADS - 1) / oa::VOX_THREADS);
    const int width = bits <= 32 ? bits : 30;
    DevTmp<uint32_t> part;
    DevTmp<int> prev;
    HIPCHK(part.alloc((size_t)n)); HIPCHK(order.alloc((size_t)n));
    if (bits > width) HIPCHK(prev.alloc((size_t)n));
    for (int shift = 0; shift < bits; shift += width) {
        const int w = std::min(width, bits - shift);
        const unsigned mask = w >= 32 ? 0xFFFFFFFFu : ((1u << w) - 1u);
        hipLaunchKernelGGL(oa::k_voxel_key_part, dim3(blocks), dim3(oa::VOX_THREADS), 0, c->stream, d_keys, n, shift, mask, part.p);
        HIPCHK(hipGetLastError());
        if (shift) std::swap(order.p, prev.p);
        const int rc = shift ? lex_order_next(c, part.p, w, prev.p, order.p, (size_t)n) : sort_order_bits(c, part.p, order.p, (size_t)n, w);
        if (rc) return rc;
    }
    return OA_OK;
}
}  // namespace

OA_EXPORT int oa_voxel_downsample(oa_ctx *c, const float *xyz, int64_t n, int on_device, const float *normals, double voxel, const double origin[3],
                                  int64_t cap, float *out_xyz, float *out_normals, int32_t *out_count, int64_t *out_rep, int64_t *n_out, oa_voxel_report *rep)
{
    if (!c || !xyz) return fail(OA_E_BAD_ARG, "oa_voxel_downsample: null argument");
    OA_NOT_MULTI(c, "oa_voxel_downsample");
    if (!(voxel > 0.0) || !(voxel < (double)INFINITY)) return fail(OA_E_BAD_ARG, "oa_voxel_downsample: voxel = %g (finite and > 0)", voxel);
    if (n < 1 || n > (int64_t)oa::SORT_MAX_N) return fail(OA_E_BAD_ARG, "oa_voxel_downsample: %lld points (1 .. 2^31 - 2^20)", (long long)n);
    if (normals && !out_normals) return fail(OA_E_BAD_ARG, "oa_voxel_downsample: normals given and nowhere to put the rows' normals");
    if (origin)
        for (int a = 0; a < 3; ++a)
            if (!(fabs(origin[a]) < (double)INFINITY)) return fail(OA_E_BAD_ARG, "oa_voxel_downsample: origin[%d] = %g", a, origin[a]);
    if (cap < 0) cap = 0;
    int rc = use_device(c);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    oa_voxel_report r;
    memset(&r, 0, sizeof r);
    r.n_in = n;
    if (n_out) *n_out = 0;
    if (rep) *rep = r;
    const int ni = (int)n;
    const unsigned pt_blocks = (unsigned)(((size_t)n + oa::VOX_THREADS - 1) / oa::VOX_THREADS);
    DevTmp<float> tmp_xyz, tmp_nrm;
    const float *d_xyz = nullptr, *d_nrm = nullptr;
    if ((rc = stage_floats(c, xyz, 3 * (size_t)n, on_device, tmp_xyz, d_xyz))) return rc;
    if (normals && (rc = stage_floats(c, normals, 3 * (size_t)n, on_device, tmp_nrm, d_nrm))) return rc;
    // 1. the box of the finite points and their number
    oa::VoxelGrid g{};
    long long dims[3];
    {
        const int nb = (int)std::min<long long>(oa::VOX_BBOX_BLOCKS, pt_blocks);
        DevTmp<float> d_bb;
        DevTmp<int> d_cnt;
        HIPCHK(d_bb.alloc(6 * (size_t)nb)); HIPCHK(d_cnt.alloc((size_t)nb));
        hipLaunchKernelGGL(oa::k_voxel_bbox, dim3((unsigned)nb), dim3(oa::VOX_THREADS), 0, c->stream, d_xyz, ni, d_bb.p, d_cnt.p);
        HIPCHK(hipGetLastError());
        std::vector<float> bb(6 * (size_t)nb);
        std::vector<int> cnt((size_t)nb);
        HIPCHK(hipMemcpyAsync(bb.data(), d_bb.p, sizeof(float) * bb.size(), hipMemcpyDeviceToHost, c->stream));
        if ((rc = read_small(c, cnt.data(), d_cnt.p, sizeof(int) * cnt.size()))) return rc;
        float lo[3], hi[3];
        (void)fold_bbox(bb.data(), nb, lo, hi);                      // (k_voxel_bbox leaves the non-finite points out)
        for (int b = 0; b < nb; ++b) r.n_finite += cnt[(size_t)b];
        if (rep) *rep = r;
        if (r.n_finite < 1) return fail(OA_E_BAD_ARG, "oa_voxel_downsample: none of the %lld points has three finite coordinates", (long long)n);
        g.h = voxel;
        for (int a = 0; a < 3; ++a) {
            g.o[a] = origin ? origin[a] : (double)lo[a];
            r.origin[a] = g.o[a];
            // floor, the division by voxel > 0 and the subtraction are monotone: the extreme cells are the extreme coordinates'
            const double c_lo = voxel_cell_of(lo[a], g.o[a], voxel), c_hi = voxel_cell_of(hi[a], g.o[a], voxel);
            if (c_lo < 0.0) return fail(OA_E_BAD_ARG, "oa_voxel_downsample: a point lies below the origin on axis %d (%g < %g)", a, (double)lo[a], g.o[a]);
            if (!(c_hi + 1.0 <= (double)oa::VOX_MAX_DIM))
                return fail(OA_E_BAD_ARG, "oa_voxel_downsample: %g cells on axis %d (at most %d: use a larger voxel)", c_hi + 1.0, a, oa::VOX_MAX_DIM);
            dims[a] = (long long)c_hi + 1;
            r.dims[a] = (int32_t)dims[a];
        }
        g.dx = dims[0]; g.dy = dims[1];
        if (rep) *rep = r;
    }
    const int nf = (int)r.n_finite;
    // 2., 3. keys and their stable order; the points that take no part carry the all-ones key and sort last: `bits` is what the
    // number of cells itself needs, so that the all-ones slice is above every cell's
    const unsigned long long cells = (unsigned long long)dims[0] * (unsigned long long)dims[1] * (unsigned long long)dims[2];   // <= 2^63
    int bits = 1;
    while (bits < 64 && (cells >> bits) != 0ull) ++bits;
    DevTmp<unsigned long long> d_keys;
    DevTmp<int> d_order;
    HIPCHK(d_keys.alloc((size_t)n));
    hipLaunchKernelGGL(oa::k_voxel_keys, dim3(pt_blocks), dim3(oa::VOX_THREADS), 0, c->stream, d_xyz, ni, g, d_keys.p);
    HIPCHK(hipGetLastError());
    if ((rc = voxel_sort_keys(c, d_keys.p, ni, bits, d_order))) return rc;
    // 4. rows
    const unsigned f_blocks = (unsigned)(((size_t)nf + oa::VOX_THREADS - 1) / oa::VOX_THREADS);
    DevTmp<int> d_head;
    DevTmp<long long> d_off;
    DevTmp<char> scan_tmp, scan_tmp2;
    HIPCHK(d_head.alloc((size_t)nf)); HIPCHK(d_off.alloc((size_t)nf + 1));
    hipLaunchKernelGGL(oa::k_voxel_heads, dim3(f_blocks), dim3(oa::VOX_THREADS), 0, c->stream, (const unsigned long long *)d_keys.p, (const int *)d_order.p, nf, d_head.p);
    HIPCHK(hipGetLastError());
    if ((rc = scan_counts(c, d_head.p, nf, d_off.p, scan_tmp))) return rc;
    long long n_rows = 0;
    if ((rc = read_small(c, &n_rows, d_off.p + nf, sizeof n_rows))) return rc;
    if (n_rows < 1 || n_rows > nf) return fail(OA_E_HIP, "oa_voxel_downsample: %lld rows from %d points", n_rows, nf);
    const int nr = (int)n_rows;
    const unsigned r_blocks = (unsigned)(((size_t)nr + oa::VOX_THREADS - 1) / oa::VOX_THREADS);
    const unsigned g_blocks = (unsigned)(((size_t)nr * oa::VOX_GROUP + oa::VOX_THREADS - 1) / oa::VOX_THREADS);
    const size_t max_chunks = oa::voxel_max_chunks((size_t)nf);
    const unsigned l_blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((max_chunks + 3) / 4, (size_t)c->n_cu * 16));
    DevTmp<int> d_row_start, d_nchunks, d_count, d_rep, d_max, d_pidx;
    DevTmp<long long> d_chunk_off;
    DevTmp<double> d_partial, d_pd2;
    DevTmp<float> d_oxyz, d_onrm;
    HIPCHK(d_row_start.alloc((size_t)nr + 1)); HIPCHK(d_nchunks.alloc((size_t)nr)); HIPCHK(d_chunk_off.alloc((size_t)nr + 1));
    HIPCHK(d_count.alloc((size_t)nr)); HIPCHK(d_rep.alloc((size_t)nr)); HIPCHK(d_max.alloc(1));
    HIPCHK(d_partial.alloc(6 * max_chunks)); HIPCHK(d_pd2.alloc(max_chunks)); HIPCHK(d_pidx.alloc(max_chunks));
    HIPCHK(d_oxyz.alloc(3 * (size_t)nr));
    if (d_nrm) HIPCHK(d_onrm.alloc(3 * (size_t)nr));
    HIPCHK(hipMemsetAsync(d_max.p, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(oa::k_voxel_row_start, dim3(f_blocks), dim3(oa::VOX_THREADS), 0, c->stream, (const int *)d_head.p, (const long long *)d_off.p, nf, d_row_start.p);
    hipLaunchKernelGGL(oa::k_voxel_row_chunks, dim3(r_blocks), dim3(oa::VOX_THREADS), 0, c->stream, (const int *)d_row_start.p, nr, d_nchunks.p);
    HIPCHK(hipGetLastError());
    if ((rc = scan_counts(c, d_nchunks.p, nr, d_chunk_off.p, scan_tmp2))) return rc;
    // 5. means and normals: short rows, long rows' chunks, long rows' chunk sums in chunk order
    hipLaunchKernelGGL(oa::k_voxel_reduce, dim3(g_blocks), dim3(oa::VOX_THREADS), 0, c->stream, d_xyz, d_nrm, (const int *)d_order.p, (const int *)d_row_start.p, nr,
                       d_oxyz.p, d_onrm.p, d_count.p, d_max.p);
    hipLaunchKernelGGL(oa::k_voxel_reduce_long, dim3(l_blocks), dim3(oa::VOX_THREADS), 0, c->stream, d_xyz, d_nrm, (const int *)d_order.p, (const int *)d_row_start.p,
                       (const long long *)d_chunk_off.p, nr, d_partial.p);
    hipLaunchKernelGGL(oa::k_voxel_finish_long, dim3(r_blocks), dim3(oa::VOX_THREADS), 0, c->stream, (const int *)d_row_start.p, (const long long *)d_chunk_off.p, nr,
                       (const double *)d_partial.p, d_nrm != nullptr, d_oxyz.p, d_onrm.p);
    HIPCHK(hipGetLastError());
    // 6. representatives, against the rounded means
    hipLaunchKernelGGL(oa::k_voxel_rep, dim3(g_blocks), dim3(oa::VOX_THREADS), 0, c->stream, d_xyz, (const int *)d_order.p, (const int *)d_row_start.p, nr,
                       (const float *)d_oxyz.p, d_rep.p);
    hipLaunchKernelGGL(oa::k_voxel_rep_long, dim3(l_blocks), dim3(oa::VOX_THREADS), 0, c->stream, d_xyz, (const int *)d_order.p, (const int *)d_row_start.p,
                       (const long long *)d_chunk_off.p, nr, (const float *)d_oxyz.p, d_pd2.p, d_pidx.p);
    hipLaunchKernelGGL(oa::k_voxel_rep_finish_long, dim3(r_blocks), dim3(oa::VOX_THREADS), 0, c->stream, (const long long *)d_chunk_off.p, nr, (const double *)d_pd2.p,
                       (const int *)d_pidx.p, d_rep.p);
    HIPCHK(hipGetLastError());
    // 7. out
    const bool fits = cap >= n_rows;
    std::vector<int> h_rep;
    if (fits) {
        if (out_xyz) HIPCHK(hipMemcpyAsync(out_xyz, d_oxyz.p, sizeof(float) * 3 * (size_t)nr, hipMemcpyDeviceToHost, c->stream));
        if (out_normals && d_nrm) HIPCHK(hipMemcpyAsync(out_normals, d_onrm.p, sizeof(float) * 3 * (size_t)nr, hipMemcpyDeviceToHost, c->stream));
        if (out_count) HIPCHK(hipMemcpyAsync(out_count, d_count.p, sizeof(int32_t) * (size_t)nr, hipMemcpyDeviceToHost, c->stream));
        if (out_rep) { h_rep.resize((size_t)nr); HIPCHK(hipMemcpyAsync(h_rep.data(), d_rep.p, sizeof(int) * (size_t)nr, hipMemcpyDeviceToHost, c->stream)); }
    }
    int max_members = 0;
    if ((rc = read_small(c, &max_members, d_max.p, sizeof max_members))) return rc;      // (waits for everything above)
    if (fits && out_rep) for (size_t k = 0; k < (size_t)nr; ++k) out_rep[k] = (int64_t)h_rep[k];
    r.n_voxels = n_rows;
    r.max_members = max_members;
    r.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (n_out) *n_out = n_rows;
    if (rep) *rep = r;
    if (!fits) return fail(OA_E_CAPACITY, "oa_voxel_downsample: %lld occupied voxels, room for %lld rows", n_rows, (long long)cap);
    return OA_OK;
}

// ================================================================================================
// normal-space sampling and the stability report (EXTENSION; oa_sample.hpp)
// ================================================================================================
OA_EXPORT int oa_normal_space_sample(oa_ctx *c, const float *normals, int64_t n, int on_device, int64_t m, int32_t grid, int32_t unoriented, uint32_t seed,
                                     int64_t cap, int64_t *out_idx, int32_t *out_bin, int64_t *n_out, oa_sample_report *rep)
{
    if (!c || !normals) return fail(OA_E_BAD_ARG, "oa_normal_space_sample: null argument");
    OA_NOT_MULTI(c, "oa_normal_space_sample");
    if (m < 1) return fail(OA_E_BAD_ARG, "oa_normal_space_sample: m = %lld points wanted (>= 1)", (long long)m);
    if (grid < 1 || grid > oa::NSS_MAX_GRID) return fail(OA_E_BAD_ARG, "oa_normal_space_sample: grid = %d (1 .. %d)", (int)grid, oa::NSS_MAX_GRID);
    if (n < 1 || n > (int64_t)oa::SORT_MAX_N) return fail(OA_E_BAD_ARG, "oa_normal_space_sample: %lld normals (1 .. 2^31 - 2^20)", (long long)n);
    if (cap < 0 || !out_idx) cap = 0;
    int rc = use_device(c);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    oa_sample_report r;
    memset(&r, 0, sizeof r);
    r.n_in = n;
    if (n_out) *n_out = 0;
    if (rep) *rep = r;
    const int ni = (int)n, G = (int)grid, n_bins = (unoriented ? 3 : 6) * G * G;
    const size_t sn = (size_t)n;
    const long long room = (long long)std::min<int64_t>(m, n);     // the most rows there can be
    const unsigned pt_blocks = (unsigned)((sn + oa::NSS_THREADS - 1) / oa::NSS_THREADS);
    DevTmp<float> tmp_nrm;
    const float *d_nrm = nullptr;
    if ((rc = stage_floats(c, normals, 3 * sn, on_device, tmp_nrm, d_nrm))) return rc;
    // 1. bins and hash keys
    DevTmp<int> d_bin, d_by_hash, d_order, d_counts, d_share, d_flag;
    DevTmp<uint32_t> d_bin_key, d_hash;
    DevTmp<long long> d_start, d_off, d_out;
    DevTmp<oa::NssInfo> d_info;
    DevTmp<char> scan_tmp;
    HIPCHK(d_bin.alloc(sn)); HIPCHK(d_bin_key.alloc(sn)); HIPCHK(d_hash.alloc(sn));
    HIPCHK(d_by_hash.alloc(sn)); HIPCHK(d_order.alloc(sn));
    HIPCHK(d_counts.alloc((size_t)n_bins)); HIPCHK(d_share.alloc((size_t)n_bins)); HIPCHK(d_start.alloc((size_t)n_bins));
    HIPCHK(d_flag.alloc(sn)); HIPCHK(d_off.alloc(sn + 1)); HIPCHK(d_out.alloc((size_t)room)); HIPCHK(d_info.alloc(1));
    hipLaunchKernelGGL(oa::k_nss_keys, dim3(pt_blocks), dim3(oa::NSS_THREADS), 0, c->stream, d_nrm, ni, G, unoriented ? 1 : 0, seed, n_bins, d_bin.p, d_bin_key.p,
                       d_hash.p);
    HIPCHK(hipGetLastError());
    // 2. the order (bin, hash): by hash, then stably by bin
    if ((rc = sort_order_bits(c, d_hash.p, d_by_hash.p, sn, 32))) return rc;
    if ((rc = lex_order_next(c, d_bin_key.p, bits_for((long long)n_bins + 1), d_by_hash.p, d_order.p, sn))) return rc;
    // 3., 4. the bins' counts, the level and every bin's share
    HIPCHK(hipMemsetAsync(d_counts.p, 0, sizeof(int) * (size_t)n_bins, c->stream));
    hipLaunchKernelGGL(oa::k_nss_hist, dim3(std::min<unsigned>(pt_blocks, oa::NSS_HIST_BLOCKS)), dim3(oa::NSS_THREADS), 0, c->stream, (const int *)d_bin.p, ni, n_bins,
                       d_counts.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(oa::k_nss_level, dim3(1), dim3(oa::NSS_LEVEL_THREADS), 0, c->stream, (const int *)d_counts.p, n_bins, (long long)m, d_share.p, d_start.p,
                       d_info.p);
    HIPCHK(hipGetLastError());
    // 5., 6. the points taken, then their indices in ascending order
    HIPCHK(hipMemsetAsync(d_flag.p, 0, sizeof(int) * sn, c->stream));
    hipLaunchKernelGGL(oa::k_nss_flag, dim3(pt_blocks), dim3(oa::NSS_THREADS), 0, c->stream, (const int *)d_order.p, (const int *)d_bin.p, ni, n_bins,
                       (const int *)d_share.p, (const long long *)d_start.p, d_flag.p);
    HIPCHK(hipGetLastError());
    if ((rc = scan_counts(c, d_flag.p, ni, d_off.p, scan_tmp))) return rc;
    hipLaunchKernelGGL(oa::k_nss_compact, dim3(pt_blocks), dim3(oa::NSS_THREADS), 0, c->stream, (const int *)d_flag.p, (const long long *)d_off.p, ni, room, d_out.p,
                       d_info.p);
    HIPCHK(hipGetLastError());
    oa::NssInfo info;
    if ((rc = read_small(c, &info, d_info.p, sizeof info))) return rc;                   // (waits for everything above)
    r.n_eligible = info.n_eligible; r.bins_occupied = info.bins_occupied; r.level = info.level; r.max_bin_count = info.max_bin_count;
    r.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rep) *rep = r;
    if (info.n_eligible < 1) return fail(OA_E_BAD_ARG, "oa_normal_space_sample: none of the %lld normals is finite and of length > 0", (long long)n);
    if (info.n_eligible > n || info.n_out != std::min<long long>((long long)m, info.n_eligible))
        return fail(OA_E_HIP, "oa_normal_space_sample: %lld rows for m = %lld of %lld eligible points", info.n_out, (long long)m, info.n_eligible);
    if (n_out) *n_out = info.n_out;
    if (cap < info.n_out) return fail(OA_E_CAPACITY, "oa_normal_space_sample: %lld points given, room for %lld", info.n_out, (long long)cap);
    static_assert(sizeof(long long) == sizeof(int64_t), "out_idx is copied as it is");
    HIPCHK(hipMemcpyAsync(out_idx, d_out.p, sizeof(int64_t) * (size_t)info.n_out, hipMemcpyDeviceToHost, c->stream));
    if (out_bin) HIPCHK(hipMemcpyAsync(out_bin, d_bin.p, sizeof(int32_t) * sn, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    r.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rep) *rep = r;
    return OA_OK;
}

OA_EXPORT int oa_stability(oa_ctx *c, const float *xyz, const float *normals, int64_t n, int on_device, const int64_t *idx, int64_t n_idx, oa_stability_report *rep)
{
    if (!c || !xyz || !normals || !rep) return fail(OA_E_BAD_ARG, "oa_stability: null argument");
    OA_NOT_MULTI(c, "oa_stability");
    if (n < 1 || n > (int64_t)oa::SORT_MAX_N) return fail(OA_E_BAD_ARG, "oa_stability: %lld points (1 .. 2^31 - 2^20)", (long long)n);
    if (idx) {
        if (n_idx < 1 || n_idx > (int64_t)oa::SORT_MAX_N) return fail(OA_E_BAD_ARG, "oa_stability: %lld indices (1 .. 2^31 - 2^20)", (long long)n_idx);
        for (int64_t k = 0; k < n_idx; ++k)
            if (idx[k] < 0 || idx[k] >= n) return fail(OA_E_BAD_ARG, "oa_stability: idx[%lld] = %lld outside 0 .. %lld", (long long)k, (long long)idx[k], (long long)n - 1);
    }
    int rc = use_device(c);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    memset(rep, 0, sizeof *rep);
    const long long n_used = idx ? (long long)n_idx : (long long)n;
    DevTmp<float> tmp_xyz, tmp_nrm;
    const float *d_xyz = nullptr, *d_nrm = nullptr;
    DevTmp<long long> d_idx, d_pcount;
    DevTmp<double> d_partial;
    DevTmp<oa::StabOut> d_st;
    std::vector<float> rows_xyz, rows_nrm;                          // (alive until the stream has been waited for)
    const long long *d_sel = nullptr;
    if (idx && !on_device) {
        // host arrays and a list: only the listed rows go up, in the list's order -- the same terms at the same positions, so the
        // same sums as through the index (the order of summation depends on the number of points analysed alone)
        rows_xyz.resize(3 * (size_t)n_idx); rows_nrm.resize(3 * (size_t)n_idx);
        for (size_t k = 0; k < (size_t)n_idx; ++k)
            for (int a = 0; a < 3; ++a) {
                rows_xyz[3 * k + a] = xyz[3 * (size_t)idx[k] + a];
                rows_nrm[3 * k + a] = normals[3 * (size_t)idx[k] + a];
            }
        if ((rc = stage_floats(c, rows_xyz.data(), rows_xyz.size(), 0, tmp_xyz, d_xyz))) return rc;
        if ((rc = stage_floats(c, rows_nrm.data(), rows_nrm.size(), 0, tmp_nrm, d_nrm))) return rc;
    } else {
        if ((rc = stage_floats(c, xyz, 3 * (size_t)n, on_device, tmp_xyz, d_xyz))) return rc;
        if ((rc = stage_floats(c, normals, 3 * (size_t)n, on_device, tmp_nrm, d_nrm))) return rc;
        if (idx) {                                                  // a device-resident cloud is read through the list
            static_assert(sizeof(long long) == sizeof(int64_t), "idx is copied as it is");
            HIPCHK(d_idx.alloc((size_t)n_idx));
            HIPCHK(hipMemcpyAsync(d_idx.p, idx, sizeof(int64_t) * (size_t)n_idx, hipMemcpyHostToDevice, c->stream));
            d_sel = d_idx.p;
        }
    }
    const int nb = (int)std::min<long long>(oa::STAB_MAX_BLOCKS, (n_used + oa::STAB_THREADS - 1) / oa::STAB_THREADS);   // (part of the summation order)
    HIPCHK(d_partial.alloc((size_t)nb * oa::STAB_NT)); HIPCHK(d_pcount.alloc((size_t)nb)); HIPCHK(d_st.alloc(1));
    HIPCHK(hipMemsetAsync(d_st.p, 0, sizeof(oa::StabOut), c->stream));
    for (int phase = 0; phase < 3; ++phase) {
        if (phase == 0)
            hipLaunchKernelGGL(oa::k_stab_accum<0>, dim3((unsigned)nb), dim3(oa::STAB_THREADS), 0, c->stream, d_xyz, d_nrm, d_sel, n_used, (const oa::StabOut *)d_st.p,
                               d_partial.p, d_pcount.p);
        else if (phase == 1)
            hipLaunchKernelGGL(oa::k_stab_accum<1>, dim3((unsigned)nb), dim3(oa::STAB_THREADS), 0, c->stream, d_xyz, d_nrm, d_sel, n_used, (const oa::StabOut *)d_st.p,
                               d_partial.p, d_pcount.p);
        else
            hipLaunchKernelGGL(oa::k_stab_accum<2>, dim3((unsigned)nb), dim3(oa::STAB_THREADS), 0, c->stream, d_xyz, d_nrm, d_sel, n_used, (const oa::StabOut *)d_st.p,
                               d_partial.p, d_pcount.p);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(oa::k_stab_join, dim3(1), dim3(64), 0, c->stream, (const double *)d_partial.p, (const long long *)d_pcount.p, nb, phase, d_st.p);
        HIPCHK(hipGetLastError());
    }
    oa::StabOut st;
    if ((rc = read_small(c, &st, d_st.p, sizeof st))) return rc;                         // (waits for everything above: the host's rows and idx included)
    rep->n_used = st.n_used;
    rep->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (st.n_used < 1) return fail(OA_E_BAD_ARG, "oa_stability: none of the %lld points has finite coordinates and a finite normal of length > 0", n_used);
    for (int a = 0; a < 3; ++a) rep->centroid[a] = st.c[a];
    rep->scale = st.s;
    memcpy(rep->C, st.C, sizeof st.C);
    memcpy(rep->eigenvalues, st.eig, sizeof st.eig);
    memcpy(rep->eigenvectors, st.vec, sizeof st.vec);
    rep->rank = st.rank;
    rep->cond = st.cond;
    rep->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return OA_OK;
}

// ================================================================================================
// deviation report (EXTENSION; oa_deviation.hpp)
// ================================================================================================
namespace {
// the stable order of the mesh's 3 n_tris corners by vertex: a CSR row per vertex, ascending by (triangle, corner).  Once per
// upload, shared by the pseudo-normals and the boundary masks (both walk the rows)
int ensure_corner_rows(oa_ctx *c)
{
    if (c->tgt.corner_ok) return OA_OK;
    const size_t n_corners = 3 * (size_t)c->tgt.n_tris, nv = (size_t)c->tgt.nt;
    if (n_corners > (size_t)oa::SORT_MAX_N) return fail(OA_E_CAPACITY, "the mesh's corner rows: %zu corners (the sort takes fewer than 2^31 - 2^20)", n_corners);
    HIPCHK(dev_malloc(&c->tgt.d_corner_order, sizeof(int) * n_corners));
    HIPCHK(dev_malloc(&c->tgt.d_corner_row, sizeof(long long) * (nv + 1)));
    // (the indices were checked at upload: all in 0 .. nt - 1, so they are their own keys; oa_sort.hpp adds 10-bit passes as the bits ask)
    const int rc = sort_order_bits(c, (const unsigned *)c->tgt.d_tris, c->tgt.d_corner_order, n_corners, bits_for((long long)nv));
    if (rc) return rc;
    hipLaunchKernelGGL(oa::k_pn_row_start, dim3((unsigned)((nv + 1 + 255) / 256)), dim3(256), 0, c->stream, (const int *)c->tgt.d_tris, (const int *)c->tgt.d_corner_order,
                       (long long)n_corners, (int)nv, c->tgt.d_corner_row);
    HIPCHK(hipGetLastError());
    c->tgt.corner_ok = true;
    return OA_OK;
}

// the mesh's pseudo-normals, once per upload: face normals and corner angles, the corner rows, then one thread per vertex and
// per (triangle, edge)
int ensure_pseudonormals(oa_ctx *c)
{
    if (c->tgt.pn_ok) return OA_OK;
    if (!c->tgt.surface || !c->tgt.d_tris || c->tgt.n_tris < 1 || c->tgt.nt < 1) return fail(OA_E_STATE, "pseudo-normals need a mesh target (oa_set_target_mesh)");
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n_tris = (size_t)c->tgt.n_tris, n_corners = 3 * n_tris, nv = (size_t)c->tgt.nt;
    HIPCHK(dev_malloc(&c->tgt.d_pn_face, sizeof(double) * 3 * n_tris));
    HIPCHK(dev_malloc(&c->tgt.d_pn_vertex, sizeof(float) * 3 * nv));
    HIPCHK(dev_malloc(&c->tgt.d_pn_edge, sizeof(float) * 9 * n_tris));
    DevTmp<double> d_angle;
    HIPCHK(d_angle.alloc(n_corners));
    const unsigned t_blocks = (unsigned)((n_tris + 255) / 256), c_blocks = (unsigned)((n_corners + 255) / 256);
    hipLaunchKernelGGL(oa::k_pn_face, dim3(t_blocks), dim3(256), 0, c->stream, (const float *)c->tgt.d_tgt_xyz, (const int *)c->tgt.d_tris, (int)n_tris, c->tgt.d_pn_face,
                       d_angle.p);
    HIPCHK(hipGetLastError());
    const int rc = ensure_corner_rows(c);
    if (rc) return rc;
    hipLaunchKernelGGL(oa::k_pn_vertex, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, c->stream, (const int *)c->tgt.d_corner_order, (const long long *)c->tgt.d_corner_row, (int)nv,
                       (const double *)c->tgt.d_pn_face, (const double *)d_angle.p, c->tgt.d_pn_vertex);
    hipLaunchKernelGGL(oa::k_pn_edge, dim3(c_blocks), dim3(256), 0, c->stream, (const int *)c->tgt.d_tris, (int)n_tris, (const int *)c->tgt.d_corner_order,
                       (const long long *)c->tgt.d_corner_row, (const double *)c->tgt.d_pn_face, c->tgt.d_pn_edge);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));                        // (the temporaries go back to the cache behind this)
    c->tgt.pn_ok = true;
    c->last_pn_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return OA_OK;
}

// the set bits of a mask, counted on the device (k_boundary_count)
int boundary_count(oa_ctx *c, const unsigned char *d_mask, size_t n, long long &out)
{
    DevTmp<unsigned> d_n;
    HIPCHK(d_n.alloc(1));
    HIPCHK(hipMemsetAsync(d_n.p, 0, sizeof(unsigned), c->stream));
    const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((n + oa::BND_THREADS - 1) / oa::BND_THREADS, 256));   // (one atomic per wave on one word)
    hipLaunchKernelGGL(oa::k_boundary_count, dim3(blocks), dim3(oa::BND_THREADS), 0, c->stream, d_mask, (long long)n, d_n.p);
    HIPCHK(hipGetLastError());
    unsigned h = 0;
    const int rc = read_small(c, &h, d_n.p, sizeof h);
    if (rc) return rc;
    out = (long long)h;
    return OA_OK;
}
}  // namespace

namespace {
// the target's boundary masks (oa_boundary.hpp), built on the context's stream and kept: a mesh's until the next upload, a cloud's
// also until its normals or (k, angle_deg) change.  The device and the stream are the caller's (use_device); no loop is running
int ensure_boundary(oa_ctx *c, int k, double angle_deg)
{
    if (c->tgt.nt <= 0) return fail(OA_E_STATE, "the target's boundary: call oa_set_target or oa_set_target_mesh first");
    if (c->tgt.surface) {
        if (c->tgt.bnd_ok) return OA_OK;
        if (!c->tgt.d_tris || c->tgt.n_tris < 1) return fail(OA_E_STATE, "the target's boundary: the mesh has no triangles");
    } else {
        if (!c->tgt.d_tgt_n)
            return fail(OA_E_STATE, "the boundary of a point-cloud target needs its normals: call oa_set_target_normals (or oa_set_normals, or install an estimate) first");
        const int rcp = check_boundary_params("the target's boundary", k, angle_deg, c->tgt.nt);
        if (rcp) return rcp;
        if (c->tgt.bnd_ok && c->tgt.bnd_built_k == k && c->tgt.bnd_built_angle == angle_deg && c->tgt.bnd_built_r2 == neighbor_r2(c)) return OA_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    c->tgt.bnd_ok = false;
    const size_t nv = (size_t)c->tgt.nt;
    if (!c->tgt.d_bnd_vmask) HIPCHK(dev_malloc(&c->tgt.d_bnd_vmask, nv));
    int rc;
    if (c->tgt.surface) {
        const size_t n_tris = (size_t)c->tgt.n_tris;
        if (!c->tgt.d_bnd_emask) HIPCHK(dev_malloc(&c->tgt.d_bnd_emask, n_tris));
        if ((rc = ensure_corner_rows(c))) return rc;
        HIPCHK(hipMemsetAsync(c->tgt.d_bnd_vmask, 0, nv, c->stream));
        constexpr size_t per_block = (size_t)(oa::BND_EDGES_PER_WAVE / 3) * (oa::BND_THREADS / 64);
        hipLaunchKernelGGL(oa::k_mesh_boundary, dim3((unsigned)((n_tris + per_block - 1) / per_block)), dim3(oa::BND_THREADS), 0, c->stream, (const int *)c->tgt.d_tris,
                           (int)n_tris, (const int *)c->tgt.d_corner_order, (const long long *)c->tgt.d_corner_row, c->tgt.d_bnd_emask, c->tgt.d_bnd_vmask);
        HIPCHK(hipGetLastError());
        if ((rc = boundary_count(c, c->tgt.d_bnd_emask, n_tris, c->tgt.bnd_n_edges))) return rc;
    } else {
        KnnTree tree;
        if ((rc = knn_tree(c, tree))) return rc;
        DevTmp<int32_t> d_idx;
        HIPCHK(d_idx.alloc(nv * (size_t)(k + 1)));
        if ((rc = knn_launch<false>(c, tree, k + 1, neighbor_r2(c), d_idx.p, nullptr, oa::KnnOrient{}, nullptr, nullptr))) return rc;
        hipLaunchKernelGGL(oa::k_cloud_boundary, dim3(wave_blocks(c, c->tgt.nt, oa::BND_WPB)), dim3(oa::BND_WPB * 64), 0, c->stream, (const float *)c->tgt.d_tgt_xyz, (const float *)c->tgt.d_tgt_n,
                           (const int32_t *)d_idx.p, c->tgt.nt, k, angle_deg * 3.14159265358979323846 / 180.0, c->tgt.d_bnd_vmask);
        HIPCHK(hipGetLastError());
        c->tgt.bnd_n_edges = 0;
        c->tgt.bnd_built_k = k; c->tgt.bnd_built_angle = angle_deg; c->tgt.bnd_built_r2 = neighbor_r2(c);
        if ((rc = boundary_count(c, c->tgt.d_bnd_vmask, nv, c->tgt.bnd_n_vertices))) return rc;   // (waits: the temporaries go back behind it)
    }
    if (c->tgt.surface && (rc = boundary_count(c, c->tgt.d_bnd_vmask, nv, c->tgt.bnd_n_vertices))) return rc;
    c->tgt.bnd_ok = true;
    c->last_bnd_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return OA_OK;
}
}  // namespace

OA_EXPORT int oa_target_boundary(oa_ctx *c, int k, double angle_deg, uint8_t *vertex_mask, uint8_t *edge_mask)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    OA_NOT_MULTI(c, "oa_target_boundary (single-device)");
    if (c->tgt.nt <= 0) return fail(OA_E_STATE, "oa_target_boundary: call oa_set_target or oa_set_target_mesh first");
    if (!c->tgt.surface && edge_mask) return fail(OA_E_BAD_ARG, "oa_target_boundary: a point-cloud target has no edges (pass edge_mask = NULL)");
    int rc = use_device(c);
    if (rc) return rc;
    if (c->loop_active) { HIPCHK(hipStreamSynchronize(c->stream)); c->loop_active = false; }   // a running sequence ends, as with oa_target_knn
    if ((rc = ensure_boundary(c, k, angle_deg))) return rc;
    if (vertex_mask) HIPCHK(hipMemcpyAsync(vertex_mask, c->tgt.d_bnd_vmask, (size_t)c->tgt.nt, hipMemcpyDeviceToHost, c->stream));
    if (edge_mask) HIPCHK(hipMemcpyAsync(edge_mask, c->tgt.d_bnd_emask, (size_t)c->tgt.n_tris, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return OA_OK;
}

OA_EXPORT int oa_get_mesh_pseudonormals(oa_ctx *c, float *vertex_n, float *edge_n)
{
    if (!c) return fail(OA_E_BAD_ARG, "null context");
    OA_ROUTE_FIRST(c, oa_get_mesh_pseudonormals(sub, vertex_n, edge_n));   // (the target is replicated: the same bits everywhere)
    if (!c->tgt.surface || c->tgt.nt <= 0) return fail(OA_E_STATE, "oa_get_mesh_pseudonormals: no mesh target (oa_set_target_mesh)");
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = ensure_pseudonormals(c))) return rc;
    if (vertex_n) HIPCHK(hipMemcpyAsync(vertex_n, c->tgt.d_pn_vertex, sizeof(float) * 3 * (size_t)c->tgt.nt, hipMemcpyDeviceToHost, c->stream));
    if (edge_n) HIPCHK(hipMemcpyAsync(edge_n, c->tgt.d_pn_edge, sizeof(float) * 9 * (size_t)c->tgt.n_tris, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return OA_OK;
}

OA_EXPORT int oa_deviation(oa_ctx *c, const oa_deviation_settings *ds, double *signed_d, double *dist, float *closest, int64_t *idx, int8_t *feature,
                           int64_t *hist, oa_deviation_report *rep)
{
    if (!c || !ds) return fail(OA_E_BAD_ARG, "oa_deviation: null argument");
    OA_NOT_MULTI(c, "oa_deviation");
    if (!(ds->thresh > 0.0)) return fail(OA_E_BAD_THRESH, "oa_deviation: thresh = %g (> 0; +inf counts every pair)", ds->thresh);
    if (ds->signed_mode < -1 || ds->signed_mode > 1) return fail(OA_E_BAD_ARG, "oa_deviation: signed_mode %d (-1 when possible, 0 never, 1 required)", ds->signed_mode);
    if (ds->n_quantiles < 0 || ds->n_quantiles > oa::DEV_MAX_Q) return fail(OA_E_BAD_ARG, "oa_deviation: %d quantiles (0 .. %d)", ds->n_quantiles, oa::DEV_MAX_Q);
    for (int k = 0; k < ds->n_quantiles; ++k)
        if (!(ds->quantiles[k] > 0.0 && ds->quantiles[k] <= 1.0)) return fail(OA_E_BAD_ARG, "oa_deviation: quantile %g outside (0, 1]", ds->quantiles[k]);
    if (ds->n_bins < 0 || ds->n_bins > oa::DEV_MAX_BINS) return fail(OA_E_BAD_ARG, "oa_deviation: %d bins (0 .. %d)", ds->n_bins, oa::DEV_MAX_BINS);
    if (ds->n_bins > 0 && !(ds->hist_lo < ds->hist_hi && fabs(ds->hist_lo) < (double)INFINITY && fabs(ds->hist_hi) < (double)INFINITY))
        return fail(OA_E_BAD_ARG, "oa_deviation: histogram range [%g, %g) (finite, lo < hi)", ds->hist_lo, ds->hist_hi);
    int rc = check_ready(c);
    if (rc) return rc;
    int sign_mode = oa::DEV_SIGN_NONE;
    if (ds->signed_mode != 0) {
        if (c->tgt.surface) sign_mode = oa::DEV_SIGN_MESH;
        else if (c->tgt.d_tgt_n) sign_mode = oa::DEV_SIGN_VERTEX;
        else if (ds->signed_mode == 1)
            return fail(OA_E_STATE, "oa_deviation: signed distances to a point-cloud target need its normals (oa_set_target_normals, oa_set_normals or an estimate)");
    }
    if ((rc = use_device(c))) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = ensure_common(c))) return rc;
    if ((rc = ensure_events(c, 1))) return rc;
    oa_deviation_report r;
    memset(&r, 0, sizeof r);
    r.n = c->src.ns;
    r.max_index = -1;
    r.surface = c->tgt.surface ? 1 : 0;
    r.signed_used = sign_mode;
    r.n_quantiles = ds->n_quantiles;
    const double nan = std::nan("");
    r.fitness = r.mean = r.rms = r.std = r.mean_signed = r.max_dist = nan;
    for (int k = 0; k < oa::DEV_MAX_Q; ++k) r.quantile_values[k] = nan;
    const bool with_hist = hist && ds->n_bins > 0;
    if (with_hist) for (int b = 0; b < ds->n_bins + 2; ++b) hist[b] = 0;
    if (sign_mode == oa::DEV_SIGN_MESH) {
        const bool built = c->tgt.pn_ok;
        if ((rc = ensure_pseudonormals(c))) return rc;
        if (!built) r.pseudonormal_ms = c->last_pn_ms;
    }
    // the device state as oa_nn_search stages it (no search radius: every slot gets its nearest primitive); a running sequence ends
    if ((rc = push_state_for_oneshot(c, 1.0, false))) return rc;
    if (c->src.ns <= 0) { r.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); if (rep) *rep = r; return OA_OK; }
    const size_t ns = (size_t)c->src.ns;
    const int n_rows = (c->src.ns_pad + oa::DEV_THREADS - 1) / oa::DEV_THREADS, nq = ds->n_quantiles;
    DevTmp<long long> d_idx;
    DevTmp<float> d_closest;
    DevTmp<double> d_dist, d_signed;
    DevTmp<signed char> d_feature;
    DevTmp<uint32_t> d_dkeys, d_qhist;
    DevTmp<unsigned long long> d_hist;
    DevTmp<oa::DevRow> d_rows;
    DevTmp<oa::DevSelect> d_sel;
    if (idx) HIPCHK(d_idx.alloc(ns));
    if (closest) HIPCHK(d_closest.alloc(3 * ns));
    if (dist) HIPCHK(d_dist.alloc(ns));
    if (signed_d) HIPCHK(d_signed.alloc(ns));
    if (feature) HIPCHK(d_feature.alloc(ns));
    HIPCHK(d_dkeys.alloc(ns)); HIPCHK(d_rows.alloc((size_t)n_rows + 1));
    oa::DevHist hg{};
    if (with_hist) {
        hg.lo = ds->hist_lo; hg.hi = ds->hist_hi; hg.n_bins = ds->n_bins;
        hg.scale = (double)ds->n_bins / (ds->hist_hi - ds->hist_lo);
        HIPCHK(d_hist.alloc((size_t)ds->n_bins + 2));
        HIPCHK(hipMemsetAsync(d_hist.p, 0, sizeof(unsigned long long) * ((size_t)ds->n_bins + 2), c->stream));
    }
    oa::DevSelect h_sel[oa::DEV_MAX_Q];
    if (nq > 0) {
        memset(h_sel, 0, sizeof h_sel);
        for (int k = 0; k < nq; ++k) { h_sel[k].p = ds->quantiles[k]; h_sel[k].q = nan; }
        HIPCHK(d_sel.alloc((size_t)nq)); HIPCHK(d_qhist.alloc((size_t)nq * oa::SEL_LEVELS * oa::SEL_BINS));
        HIPCHK(hipMemcpyAsync(d_sel.p, h_sel, sizeof(oa::DevSelect) * (size_t)nq, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemsetAsync(d_qhist.p, 0, sizeof(uint32_t) * (size_t)nq * oa::SEL_LEVELS * oa::SEL_BINS, c->stream));
    }
    HIPCHK(hipEventRecord(c->ev[0], c->stream));
    if ((rc = launch_nn(c, choose_search(c), false))) return rc;
    HIPCHK(hipEventRecord(c->ev[1], c->stream));
    const oa::DevOut out{ d_idx.p, d_closest.p, d_dist.p, d_signed.p, d_feature.p };
    hipLaunchKernelGGL(oa::k_deviation, dim3((unsigned)n_rows), dim3(oa::DEV_THREADS), 0, c->stream, (const oa::DevState *)c->d_state, (const float4 *)c->src.d_src4,
                       c->src.ns, c->src.ns_pad, (const float *)c->tgt.d_tgt_xyz, c->src.d_keys, c->tgt.surface ? (const float4 *)nullptr : (const float4 *)c->src.d_win,
                       c->tgt.surface ? (const float4 *)c->tgt.d_tri9 : (const float4 *)nullptr, ds->thresh, sign_mode, (const int *)c->tgt.d_tris,
                       (const double *)c->tgt.d_pn_face, (const float *)c->tgt.d_pn_vertex, (const float *)c->tgt.d_pn_edge, (const float *)c->tgt.d_tgt_n,
                       (const int *)c->src.d_perm, out, d_dkeys.p, hg, with_hist ? d_hist.p : (unsigned long long *)nullptr, d_rows.p);
    hipLaunchKernelGGL(oa::k_dev_finish, dim3(1), dim3(oa::DEV_FIN_THREADS), 0, c->stream, (const oa::DevRow *)d_rows.p, n_rows, d_rows.p + n_rows);
    HIPCHK(hipGetLastError());
    if (nq > 0) {
        launch_dev_select(c, d_sel.p, nq, (const uint32_t *)d_dkeys.p, d_qhist.p, false);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_sel, d_sel.p, sizeof(oa::DevSelect) * (size_t)nq, hipMemcpyDeviceToHost, c->stream));
    }
    std::vector<unsigned long long> h_hist;
    if (with_hist) {
        h_hist.resize((size_t)ds->n_bins + 2);
        HIPCHK(hipMemcpyAsync(h_hist.data(), d_hist.p, sizeof(unsigned long long) * h_hist.size(), hipMemcpyDeviceToHost, c->stream));
    }
    if (idx) HIPCHK(hipMemcpyAsync(idx, d_idx.p, sizeof(long long) * ns, hipMemcpyDeviceToHost, c->stream));
    if (closest) HIPCHK(hipMemcpyAsync(closest, d_closest.p, sizeof(float) * 3 * ns, hipMemcpyDeviceToHost, c->stream));
    if (dist) HIPCHK(hipMemcpyAsync(dist, d_dist.p, sizeof(double) * ns, hipMemcpyDeviceToHost, c->stream));
    if (signed_d) HIPCHK(hipMemcpyAsync(signed_d, d_signed.p, sizeof(double) * ns, hipMemcpyDeviceToHost, c->stream));
    if (feature) HIPCHK(hipMemcpyAsync(feature, d_feature.p, ns, hipMemcpyDeviceToHost, c->stream));
    oa::DevRow tot;
    if ((rc = read_small(c, &tot, d_rows.p + n_rows, sizeof tot))) return rc;   // (waits for everything above)
    {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        r.search_ms = ms;
    }
    r.n_valid = tot.n_valid; r.n_inlier = tot.n_inlier; r.n_inside = tot.n_inside; r.n_unsigned = tot.n_unsigned;
    r.fitness = (double)tot.n_inlier / (double)r.n;
    if (tot.n_inlier > 0) {
        const double k = (double)tot.n_inlier;
        r.mean = tot.sum_d / k;
        r.rms = sqrt(tot.sum_dd / k);
        r.mean_signed = tot.sum_signed / k;
        const double var = r.rms * r.rms - r.mean * r.mean;
        r.std = sqrt(var > 0.0 ? var : 0.0);
    }
    if (tot.max_index >= 0) {
        r.max_index = tot.max_index;
        memcpy(&r.max_dist, &tot.max_bits, sizeof(double));
    }
    for (int k = 0; k < nq; ++k) r.quantile_values[k] = h_sel[k].q;
    if (with_hist) for (size_t b = 0; b < h_hist.size(); ++b) hist[b] = (int64_t)h_hist[b];
    r.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rep) *rep = r;
    return OA_OK;
}
