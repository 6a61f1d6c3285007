// The OA_* tuning and test hooks, read from the environment ONCE: the per-context ones when a context is created
// (oa_ctx::tune), the two of the device-block cache when the process first allocates.  Nothing else in csrc/ looks at the
// environment -- the library is a guest in somebody else's process, and a getenv on a call path, from pool threads, is not
// something it should do.  Plain C++, no HIP header: a clamp that needs a kernel header's constant stays at the use site.
#pragma once
#include <cstdlib>
#include <cstring>
#include <algorithm>

namespace oa_tune {

// unset or empty: the default
inline int env_int(const char *name, int dflt)
{
    const char *v = std::getenv(name);
    return (v && *v) ? std::atoi(v) : dflt;
}

inline double env_double(const char *name, double dflt)
{
    const char *v = std::getenv(name);
    return (v && *v) ? std::atof(v) : dflt;
}

inline bool env_is(const char *name, const char *a, const char *b = nullptr, const char *c = nullptr)
{
    const char *v = std::getenv(name);
    return v && (!std::strcmp(v, a) || (b && !std::strcmp(v, b)) || (c && !std::strcmp(v, c)));
}

constexpr int UNSET = -0x7fffffff - 1;      // "no value given" of a knob whose default is computed where it is used

struct Tunables {
    // --- search: which one, and the turns between them
    int nn_grid = -1;                // OA_NN_GRID: initial search mode, -1 auto, 0 never a grid (brute force), 1 grid whenever possible, 2 tree (oa_set_search_mode overrides)
    int search_turns = 1;            // OA_SEARCH_TURNS: tree while the pose moves, grid afterwards (mid-size shards, AUTO)
    double turn_frac = 0.1;          // OA_TURN_FRAC: the tree keeps its turn while the pose moves by more than this part of a cell
    bool nn_cutoff = true;           // OA_NN_CUTOFF=0: grid / tree searches ignore the search radius derived from thresh (same pairs, slower)
    bool no_identity_path = false;   // OA_NO_IDENTITY_PATH=1 (A/B): an identity target matrix goes through the general path too
    // --- brute force (k_nn_search_sorted and its predecessors)
    int nn_r = 0;                    // OA_NN_R: source points per thread, 1 / 2 / 4 / 8 (0 and anything else = choose from the shard size; 8 only with the experiments)
    bool nn_filter = true;           // OA_NN_FILTER=0: the exact unfiltered kernel k_nn_search
    bool nn_sort = true;             // OA_NN_SORT=0 (A/B, experiments): the brute-force search stays k_nn_search_filtered (rounds 1-4)
    bool nn_home_pass = true;        // OA_NN_HOME_PASS=0: the first search of a loop is ONE unseeded launch (else k_nn_seed_sorted + a seeded launch)
    bool nn_wave_order = true;       // OA_NN_WAVE_ORDER=0: k_nn_search_sorted's point records in the slots' own order
    bool nn_vchunk = true;           // OA_NN_VCHUNK: the sorted images' blocks in the order of v and k_nn_search_sorted's level 0v (0: as until round 6)
    int nn_persist = 4;              // OA_NN_PERSIST: workgroups per CU that work the queue off (0: one workgroup per item, in launch order -- as until round 6)
    int nn_queue_min = -1;           // OA_NN_QUEUE_MIN_ITEMS: launches of at least this many items go through the queue (-1: four per workgroup)
    bool nn_bigtile = false;         // OA_NN_BIGTILE=1: 256-group LDS tiles of k_nn_search_filtered even for small targets
    int nn_target_blocks = UNSET;    // OA_NN_TARGET_BLOCKS: workgroups wanted (unset: from the pair count, plan_geometry)
    int nn_splits = 0;               // OA_NN_SPLITS: forced number of target splits (0 = planned)
    int nn_splits_seeded = 0;        // OA_NN_SPLITS_SEEDED: ... of the seeded launches
    int nn_mfma = 0;                 // OA_NN_MFMA=1 (experiment): first filter level of the brute-force search on the matrix cores (oa_mfma.hpp)
    int mfma_wps = 4;                // OA_MFMA_WPS: waves per SIMD k_nn_search_mfma is built for (4: 128 registers, 3: 168, 2: 256)
    // --- accumulation and the loop
    int acc_blocks = 512;            // OA_ACC_BLOCKS: cap on the workgroups of k_pair_accumulate (clamped to 1..ACC_MAX_BLOCKS where it is used)
    int acc_threads = 0;             // OA_ACC_THREADS: 256 / 512 threads per workgroup of the accumulating grid search and k_pair_accumulate_canon (0 = by shard size)
    int fused_acc = 1;               // OA_FUSED_ACC: grid / tree searches of the loop accumulate in their epilogue
    int tree_acc_max = 4096;         // OA_TREE_ACC_MAX: largest shard whose whole-shard tree search also accumulates
    bool run_poll = true;            // OA_RUN_POLL=0: the loop enqueues every iteration and never waits for news from the device
    int time_events = -1;            // OA_TIME_EVENTS: hipEvent pair around every search, 0 / 1 (-1 = unset: 1 for brute force, else the GPU-side stamps)
    bool mapped_results = true;      // OA_MAPPED_RESULTS=0 (A/B): small per-workgroup results go through a device buffer + copy
    bool debug = false;              // OA_DEBUG: on when the variable exists, even empty
    // --- vertex grid (k_nn_search_grid)
    int grid_lanes = 0;              // OA_GRID_LANES: lanes per query of k_nn_search_grid (0 = by shard size)
    int grid_path = 0;               // OA_GRID_PATH=fast / safe: 0 = adaptive (see grid_fast_now), 1 = always the fused path, 2 = never
    int grid_safe = 1;               // OA_GRID_SAFE: 0 = the vertex searches (grid, whole-shard tree) never take a seed on its safe radius (A/B);
                                     // 1 = the radii are built once a target has seen SAFE_LAZY_ITERS accumulating searches (a 5-iteration
                                     // call at 1M vertices would pay 50-80 us to save 10); 2 = built with the grid
    double grid_ppc = 2.0;           // OA_GRID_PPC: target vertices per cell
    int grid_rmax = 3;               // OA_GRID_RMAX: rings a grid query scans before the tree takes it over (at most 3; both grids)
    bool grid_seeded_start = true;   // OA_GRID_SEEDED_START=0: a seeded query scans its own cell first, then the ring around it
    int grid_budget = 256;           // OA_GRID_BUDGET, vertex grid: candidates a query may look at before the tree takes it over
    double grid_budget_moving = 2.0; // OA_GRID_BUDGET_MOVING, vertex grid: factor on the budget while the pose moves
    int list_blocks_per_cu = 16;     // OA_LIST_BLOCKS_PER_CU: workgroups (of four waves) per CU of the tree search over the hand-over list
    // --- triangle grid (surface mode, oa_tri.hpp)
    int tri_budget = 192;            // OA_GRID_BUDGET, triangle grid (1..30000: range lengths are 16-bit in the kernel)
    double tri_budget_moving = 3.0;  // OA_GRID_BUDGET_MOVING, triangle grid (2.0 until the scan was shared by the wave)
    double tri_cell = 1.25;          // OA_TRI_CELL: mean triangle bbox diagonals per cell edge
    int tri_max_cells_log2 = 24;     // OA_TRI_MAX_CELLS_LOG2: cap on the triangle grid's cell count (16..29)
    bool tri_seeded_start = true;    // OA_TRI_SEEDED_START=0: as OA_GRID_SEEDED_START
    int tri_drop_over = 1;           // OA_TRI_DROP_OVER: a query whose listed cells exceed its budget scans none of them (0: scans them first; A/B)
    double tri_moving_frac = 0.25;   // OA_TRI_MOVING_FRAC: the pose "moves" above this part of a cell edge per iteration
    int tri_xcd_chunk = 8;           // OA_TRI_XCD_CHUNK: x 256 queries per XCD share (0 = contiguous shares always; at most 4096)
    double tri_xcd_moving_frac = 0.5;// OA_TRI_XCD_MOVING_FRAC: ... while the pose moves by less than this part of a cell edge
    bool tri_acc = true;             // OA_TRI_ACC=0 (A/B): the triangle grid search never accumulates in its epilogue
    bool tri_canon = true;           // OA_TRI_CANON=0 (A/B): surface loops accumulate through the grid-stride k_pair_accumulate (rounds 1-3)
    bool tri_wave_wgs = true;        // OA_TRI_WAVE_WGS=0 (A/B): the plain surface search in workgroups of 256 queries also for long launches, as until round 6
    bool tri_split_lanes = true;     // OA_TRI_SPLIT_LANES=0 (A/B): the list is always searched with the shard's own lanes per query
    bool tri_split = true;           // OA_TRI_SPLIT=0 (A/B): the seed + neighbours test stays in the grid search's prologue (no k_tri_accept launch)
    bool tri_share = true;           // OA_TRI_SHARE=0 (A/B, experiments): every lane of the triangle-grid search walks its own records (rounds 2-3)
    bool grid_stats = false;         // OA_GRID_STATS (experiments): instrumented triangle-grid launches print what the queries did
    int tri_ring = 0;                // OA_TRI_RING (EXPERIMENT, off: exact, measured, not faster -- docs/HISTORY.md 4.5): 0 = never; 1 = built once a mesh has seen TRI_RING_LAZY_ITERS searches of a loop; 2 = built with the grid
    double tri_ring_cap = 0.25;      // OA_TRI_RING_CAP: clearances are looked for up to this fraction of a cell edge
    int tri_fine = 0;                // OA_TRI_FINE (EXPERIMENT, off: measured slower than the search it fronts, docs/HISTORY.md): 0 = never, 1 = built with the mesh when it has >= tri_fine_min_tris triangles, 2 = always
    int tri_fine_min_tris = 200000;  // OA_TRI_FINE_MIN_TRIS (smaller meshes: short calls would pay ~80 us of build for a search they never reach; at least 64)
    double tri_fine_cell = 0.5;      // OA_TRI_FINE_CELL: the fine grid's cell edge in mean triangle bbox diagonals
    double tri_fine_rho = 0.3;       // OA_TRI_FINE_RHO: inflation of its lists in cell edges (0.01..4)
    double tri_fine_max_mb = 8192.0; // OA_TRI_FINE_MAX_MB: the most its records may take (at least 16)
    int tri_fine_cap = 192;          // OA_TRI_FINE_CAP: FineParams::cap (1..2^20)
    double tri_fine_gate = 1e30;     // OA_TRI_FINE_GATE: FineParams::gate in units of rho
    // --- source upload
    bool sort_source = true;         // OA_SORT_SOURCE=0: the source slots stay in the caller's order (no Morton sort, no spatial shards)
    bool shard_spatial = true;       // OA_SHARD_SPATIAL=0: shards are contiguous ranges of the selection in the caller's order
    bool partition_once = true;      // OA_PARTITION_ONCE=0 (A/B): every device of a multi-device context sorts the whole selection itself
    // --- multi-device contexts (read by the parent; the Exchange keeps its own copies, two of them are consumed by the hooks)
    bool multi_own_streams = false;  // OA_MULTI_OWN_STREAMS=1 (test hook): children that share a GPU get their own streams
    int multi_threads = -1;          // OA_MULTI_THREADS: -1 = one host thread per GPU, 0 = the calling thread only, 1 = one per child
    bool multi_agree = true;         // OA_MULTI_AGREE=0 (test hook, mailbox only): every host thread stops on its own device's flag
    int exchange = -1;               // OA_EXCHANGE=rccl|RCCL|1 / mailbox|MAILBOX|0: 1 / 0, the values of OA_EXCHANGE_RCCL / _MAILBOX (anything else: -1, _AUTO)
    double exchange_timeout_s = 30.0;// OA_EXCHANGE_TIMEOUT_S: how long a device waits for the others' sums (at least 0.05)
    bool auto_rccl_any = false;      // OA_AUTO_RCCL_ANY=1 (test hook): AUTO takes RCCL for a world of one too
    int mailbox = 0;                 // OA_MAILBOX=host / device: 1 / 2, where the mailboxes live (anything else 0 = device, host as the fallback)
    int fault_skip_post_rank = -1;   // OA_FAULT_SKIP_POST_RANK: that rank's sums never reach the mailboxes
    int fault_lag_group = -1;        // OA_FAULT_LAG_GROUP, OA_FAULT_LAG_US: a host thread that sleeps before every look at its halt flag
    int fault_lag_us = 0;
    int fault_fail_group = -1;       // OA_FAULT_FAIL_GROUP, OA_FAULT_FAIL_ITER: a host thread whose enqueue fails at an iteration
    int fault_fail_iter = -1;
    int fault_stall_rank = -1;       // OA_FAULT_STALL_RANK, OA_FAULT_STALL_ITER: a rank whose stream stops ahead of its collective
    int fault_stall_iter = 2;
};

// The one place that names the per-context variables: one line per knob, with its parse and clamp.
inline Tunables read_tunables()
{
    const Tunables d;                // the defaults, said once (above)
    Tunables t;
    t.nn_grid = env_int("OA_NN_GRID", d.nn_grid);
    t.search_turns = env_int("OA_SEARCH_TURNS", d.search_turns);
    t.turn_frac = env_double("OA_TURN_FRAC", d.turn_frac);
    t.nn_cutoff = env_int("OA_NN_CUTOFF", d.nn_cutoff) != 0;
    t.no_identity_path = env_int("OA_NO_IDENTITY_PATH", d.no_identity_path) != 0;
    t.nn_r = env_int("OA_NN_R", d.nn_r);
    if (t.nn_r != 1 && t.nn_r != 2 && t.nn_r != 4 && t.nn_r != 8) t.nn_r = 0;
    t.nn_filter = env_int("OA_NN_FILTER", d.nn_filter) != 0;
    t.nn_sort = env_int("OA_NN_SORT", d.nn_sort) != 0;
    t.nn_home_pass = env_int("OA_NN_HOME_PASS", d.nn_home_pass) != 0;
    t.nn_wave_order = env_int("OA_NN_WAVE_ORDER", d.nn_wave_order) != 0;
    t.nn_vchunk = env_int("OA_NN_VCHUNK", d.nn_vchunk) != 0;
    t.nn_persist = std::max(0, std::min(16, env_int("OA_NN_PERSIST", d.nn_persist)));
    t.nn_queue_min = env_int("OA_NN_QUEUE_MIN_ITEMS", d.nn_queue_min);
    t.nn_bigtile = env_int("OA_NN_BIGTILE", d.nn_bigtile) != 0;
    t.nn_target_blocks = env_int("OA_NN_TARGET_BLOCKS", d.nn_target_blocks);
    t.nn_splits = env_int("OA_NN_SPLITS", d.nn_splits);
    t.nn_splits_seeded = env_int("OA_NN_SPLITS_SEEDED", d.nn_splits_seeded);
    t.nn_mfma = env_int("OA_NN_MFMA", d.nn_mfma);
    t.mfma_wps = env_int("OA_MFMA_WPS", d.mfma_wps);
    t.acc_blocks = env_int("OA_ACC_BLOCKS", d.acc_blocks);
    t.acc_threads = env_int("OA_ACC_THREADS", d.acc_threads);
    t.fused_acc = env_int("OA_FUSED_ACC", d.fused_acc);
    t.tree_acc_max = env_int("OA_TREE_ACC_MAX", d.tree_acc_max);
    t.run_poll = env_int("OA_RUN_POLL", d.run_poll) != 0;
    { const int v = env_int("OA_TIME_EVENTS", UNSET); t.time_events = v == UNSET ? -1 : (v != 0 ? 1 : 0); }
    t.mapped_results = env_int("OA_MAPPED_RESULTS", d.mapped_results) != 0;
    t.debug = std::getenv("OA_DEBUG") != nullptr;
    t.grid_lanes = env_int("OA_GRID_LANES", d.grid_lanes);
    t.grid_path = env_is("OA_GRID_PATH", "fast") ? 1 : (env_is("OA_GRID_PATH", "safe") ? 2 : 0);
    t.grid_safe = std::max(0, std::min(2, env_int("OA_GRID_SAFE", d.grid_safe)));
    t.grid_ppc = env_double("OA_GRID_PPC", d.grid_ppc);
    t.grid_rmax = std::min(env_int("OA_GRID_RMAX", d.grid_rmax), 3);
    t.grid_seeded_start = env_int("OA_GRID_SEEDED_START", d.grid_seeded_start) != 0;
    t.grid_budget = env_int("OA_GRID_BUDGET", d.grid_budget);
    t.grid_budget_moving = env_double("OA_GRID_BUDGET_MOVING", d.grid_budget_moving);
    t.list_blocks_per_cu = std::max(1, std::min(64, env_int("OA_LIST_BLOCKS_PER_CU", d.list_blocks_per_cu)));
    t.tri_budget = std::max(1, std::min(env_int("OA_GRID_BUDGET", d.tri_budget), 30000));
    t.tri_budget_moving = env_double("OA_GRID_BUDGET_MOVING", d.tri_budget_moving);
    t.tri_cell = env_double("OA_TRI_CELL", d.tri_cell);
    t.tri_max_cells_log2 = std::max(16, std::min(29, env_int("OA_TRI_MAX_CELLS_LOG2", d.tri_max_cells_log2)));
    t.tri_seeded_start = env_int("OA_TRI_SEEDED_START", d.tri_seeded_start) != 0;
    t.tri_drop_over = env_int("OA_TRI_DROP_OVER", d.tri_drop_over);
    t.tri_moving_frac = env_double("OA_TRI_MOVING_FRAC", d.tri_moving_frac);
    t.tri_xcd_chunk = std::max(0, std::min(4096, env_int("OA_TRI_XCD_CHUNK", d.tri_xcd_chunk)));
    t.tri_xcd_moving_frac = env_double("OA_TRI_XCD_MOVING_FRAC", d.tri_xcd_moving_frac);
    t.tri_acc = env_int("OA_TRI_ACC", d.tri_acc) != 0;
    t.tri_canon = env_int("OA_TRI_CANON", d.tri_canon) != 0;
    t.tri_wave_wgs = env_int("OA_TRI_WAVE_WGS", d.tri_wave_wgs) != 0;
    t.tri_split_lanes = env_int("OA_TRI_SPLIT_LANES", d.tri_split_lanes) != 0;
    t.tri_split = env_int("OA_TRI_SPLIT", d.tri_split) != 0;
    t.tri_share = env_int("OA_TRI_SHARE", d.tri_share) != 0;
    t.grid_stats = env_int("OA_GRID_STATS", d.grid_stats) != 0;
    t.tri_ring = std::max(0, std::min(2, env_int("OA_TRI_RING", d.tri_ring)));
    t.tri_ring_cap = env_double("OA_TRI_RING_CAP", d.tri_ring_cap);
    t.tri_fine = std::max(0, std::min(2, env_int("OA_TRI_FINE", d.tri_fine)));
    t.tri_fine_min_tris = std::max(64, env_int("OA_TRI_FINE_MIN_TRIS", d.tri_fine_min_tris));
    t.tri_fine_cell = env_double("OA_TRI_FINE_CELL", d.tri_fine_cell);
    t.tri_fine_rho = std::max(0.01, std::min(env_double("OA_TRI_FINE_RHO", d.tri_fine_rho), 4.0));
    t.tri_fine_max_mb = std::max(16.0, env_double("OA_TRI_FINE_MAX_MB", d.tri_fine_max_mb));
    t.tri_fine_cap = std::max(1, std::min(env_int("OA_TRI_FINE_CAP", d.tri_fine_cap), 1 << 20));
    t.tri_fine_gate = env_double("OA_TRI_FINE_GATE", d.tri_fine_gate);
    t.sort_source = env_int("OA_SORT_SOURCE", d.sort_source) != 0;
    t.shard_spatial = env_int("OA_SHARD_SPATIAL", d.shard_spatial) != 0;
    t.partition_once = env_int("OA_PARTITION_ONCE", d.partition_once) != 0;
    t.multi_own_streams = env_int("OA_MULTI_OWN_STREAMS", d.multi_own_streams) != 0;
    t.multi_threads = env_int("OA_MULTI_THREADS", d.multi_threads);
    t.multi_agree = env_int("OA_MULTI_AGREE", d.multi_agree) != 0;
    t.exchange = env_is("OA_EXCHANGE", "rccl", "RCCL", "1") ? 1 : (env_is("OA_EXCHANGE", "mailbox", "MAILBOX", "0") ? 0 : -1);
    t.exchange_timeout_s = std::max(0.05, env_double("OA_EXCHANGE_TIMEOUT_S", d.exchange_timeout_s));
    t.auto_rccl_any = env_int("OA_AUTO_RCCL_ANY", d.auto_rccl_any) != 0;
    t.mailbox = env_is("OA_MAILBOX", "host") ? 1 : (env_is("OA_MAILBOX", "device") ? 2 : 0);
    t.fault_skip_post_rank = env_int("OA_FAULT_SKIP_POST_RANK", d.fault_skip_post_rank);
    t.fault_lag_group = env_int("OA_FAULT_LAG_GROUP", d.fault_lag_group);
    t.fault_lag_us = env_int("OA_FAULT_LAG_US", d.fault_lag_us);
    t.fault_fail_group = env_int("OA_FAULT_FAIL_GROUP", d.fault_fail_group);
    t.fault_fail_iter = env_int("OA_FAULT_FAIL_ITER", d.fault_fail_iter);
    t.fault_stall_rank = env_int("OA_FAULT_STALL_RANK", d.fault_stall_rank);
    t.fault_stall_iter = env_int("OA_FAULT_STALL_ITER", d.fault_stall_iter);
#if !defined(OA_EXPERIMENTS)
    // the default library does not carry the experiments (oa_families.hpp): their knobs are inert here, liboa_icp_exp.so has them
    t.nn_mfma = 0; t.tri_ring = 0; t.tri_fine = 0; t.nn_sort = true; t.grid_stats = false; t.tri_share = true;
    if (t.nn_r == 8) t.nn_r = 4;     // (8 points per thread: an OA_EXPERIMENTS instantiation)
#endif
    return t;
}

// The two process-wide knobs of the cache of released device blocks: read when the process first allocates.
struct CacheTunables {
    bool enabled = true;             // OA_DEV_CACHE: off only for a value that reads as 0 -- plain hipMalloc / hipFree
    bool cap_given = false;          // OA_DEV_CACHE_MB set: a fixed cap (else 256 MiB or the library's own peak of live bytes)
    double cap_mb = 256.0;
};

inline CacheTunables read_cache_tunables()
{
    CacheTunables t;
    const char *on = std::getenv("OA_DEV_CACHE"), *mb = std::getenv("OA_DEV_CACHE_MB");
    t.enabled = !(on && std::atoi(on) == 0);
    t.cap_given = mb && *mb;
    t.cap_mb = std::max(0.0, env_double("OA_DEV_CACHE_MB", t.cap_mb));
    return t;
}

}  // namespace oa_tune
