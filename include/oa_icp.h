/*
 * oa_icp.h -- C-ABI of liboa_icp.so: the MI355X (gfx950) ICP hot path.
 *
 * This is the drop-in boundary for the one hot path of patmo141/object_alignment
 * (SURVEY.md section 8b): what a maintainer's ctypes binding would call instead of
 *
 *   functions/general.py:257   make_pairs(align_obj, base_obj, base_bvh, vlist, thresh, sample, calc_stats)
 *   functions/general.py:105   affine_matrix_from_points(v0, v1, shear=False, scale, usesvd=True)
 *   operators/icp_align.py:96  the `while n < iters and not converged` loop of
 *                              OBJECT_OT_icp_align.execute
 *
 * Conventions
 *   - plain C, no torch / C++ types; all matrices are 4x4 ROW-major;
 *     `float` matrices carry Blender's float32 matrix_world values.
 *   - host buffers are caller-owned and only touched during the call; device
 *     buffers are library-owned and released by oa_destroy.
 *   - every function returns OA_OK (0) or a negative error code; the text of the
 *     last error on the calling thread is oa_last_error().  No C++ exception
 *     crosses this boundary.
 *   - one context = one host thread at a time (not internally locked).
 *     Multi-GPU, one process: oa_create_multi(devices, n) -- the context shards the
 *     source over the listed GPUs, replicates the target, and oa_run / oa_iterate join
 *     the devices' 24 sums inside the library every iteration.
 *     Multi-GPU, one process per GPU (torchrun, MPI): one oa_create context per rank
 *     and the split-phase loop oa_iter_partial -> all-reduce(sum) -> oa_iter_finish.
 *   - there is NO CPU fallback: every compute entry point fails with
 *     OA_E_NO_DEVICE / OA_E_HIP when no gfx950 device is usable.
 *
 * Correspondence rule: nearest target VERTEX (fp32, d2 = fma(dz,dz,fma(dy,dy,dx*dx)),
 * lowest index wins ties) -- see docs/HISTORY.md 5.3 "D2".
 */
#ifndef OA_ICP_H
#define OA_ICP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OA_OK                 0
#define OA_E_BAD_ARG         -1
#define OA_E_HIP             -2
#define OA_E_TOO_FEW_PAIRS   -3   /* K < 3: the reference raises ValueError (functions/general.py:150-157) */
#define OA_E_SINGULAR        -4   /* matrix_world not invertible (functions/general.py:265-266) */
#define OA_E_NO_DEVICE       -5
#define OA_E_STATE           -6   /* source / target / matrices not set */
#define OA_E_BAD_THRESH      -7   /* thresh <= 0: the reference returns None (functions/general.py:277) */
#define OA_E_CAPACITY        -8
#define OA_E_RCCL            -9   /* multi-device exchange failed: librccl missing / ncclCommInitAll / ncclAllReduce error,
                                     or a device's sums did not arrive within OA_EXCHANGE_TIMEOUT_S (default 30 s) -- mailbox:
                                     the waiting kernels give up by themselves; RCCL: the host's watchdog sees no device
                                     finish an iteration for that long and aborts the communicators (ncclCommAbort) */

#define OA_NSUMS 24               /* doubles exchanged per iteration (see oa_iter_partial) */

typedef struct oa_ctx oa_ctx;

/* Loop parameters: lib/preferences.py:31-72 as read at operators/icp_align.py:82-89 */
typedef struct oa_settings {
    int32_t iters;            /* icp_iterations (50) */
    int32_t use_target;       /* use_target (1): calc d_stats and run the convergence test */
    int32_t with_scale;       /* align_meth == '1' (ROT_LOC_SCALE) */
    int32_t early_exit;       /* 1 = stop when converged (reference behaviour); 0 = always run `iters` (timing runs) */
    double  thresh;           /* min_start (0.5) */
    double  target_d;         /* target_d (0.01) */
} oa_settings;

typedef struct oa_report {
    int32_t iters_done;
    int32_t converged;
    int32_t status;               /* OA_OK or the error that stopped the loop */
    int32_t reserved;
    int64_t last_K;               /* pairs used by the last iteration (all shards) */
    double  last_translation;     /* |new_mat.to_translation()| of the last iteration */
    double  mean_dist, std_dist;  /* d_stats of the last iteration (NaN when use_target = 0) */
    double  mean_rot_angle;       /* mean |rotation angle| over the last <=5 iterations (radians) */
    double  nn_ms_total;          /* hipEvent time summed over the correspondence kernels */
    double  loop_ms;              /* hipEvent time of the whole device-resident loop */
} oa_report;

/* ---- lifetime ------------------------------------------------------------------ */
int         oa_device_count(void);
int         oa_create(oa_ctx **out, int device);
/* One context over n_dev GPUs of this process (1 <= n_dev <= 64; SURVEY.md 8b's oa_create(&ctx, devices, n_dev)).
 * Every upload goes to all of them (target replicated; source: the selection is Morton-sorted ONCE, on the first
 * device, and device i receives range i of n_dev of it, see oa_set_source; the devices build their search structures
 * concurrently, one persistent host thread per GPU), oa_run hands every GPU's host thread the whole loop of its
 * device -- one stream per device, no host round trip per iteration, enqueue cost independent of n_dev -- and every
 * iteration the devices exchange their OA_NSUMS partial sums and perform the identical solve
 * (operators/icp_align.py:96-151 is still ONE call).  A device may be listed more than once (its shards then share
 * one stream and one host thread); that is how the path is tested on a single GPU.  oa_make_pairs and oa_nn_search
 * work on such a context too: every device answers for its shard and the library merges the answers back into the
 * caller's (vlist) order.  Device pointers (on_device != 0) may live on any GPU of the process: the library stages
 * them to the device that needs them.  Not available on it: oa_set_stream and the split-phase calls. */
int         oa_create_multi(oa_ctx **out, const int *devices, int n_dev);
int         oa_num_devices(oa_ctx *ctx);
/* How the devices of an oa_create_multi context join their sums (env OA_EXCHANGE=rccl / mailbox; default AUTO):
 *   OA_EXCHANGE_AUTO     RCCL when the listed devices are distinct and librccl can be brought up, else the mailbox;
 *                        decided before the first loop (OA_STAT_EXCHANGE reports the outcome)
 *   OA_EXCHANGE_RCCL     ncclAllReduce(OA_NSUMS doubles, sum) over xGMI on every device's stream, single-process
 *                        communicator (ncclCommInitAll); librccl.so.1 is loaded on first use; needs distinct devices.
 *                        New communicators first pass one all-reduce of a known vector (bounded wait) or are given up.
 *                        Every host thread enqueues the same number of collectives whatever its device reports when
 *                        (OA_STAT_ENQUEUED_MIN == _MAX); no wait for the devices is unbounded: when no device finishes an
 *                        iteration for OA_EXCHANGE_TIMEOUT_S, or RCCL reports an asynchronous error, the communicators
 *                        are aborted and the call returns OA_E_RCCL.  After that AUTO stays on the mailbox;
 *                        oa_set_exchange(OA_EXCHANGE_RCCL) builds new communicators.
 *   OA_EXCHANGE_MAILBOX  all-gather through mailboxes: every device's post is written into every device's inbox --
 *                        fine-grained device memory, peer-mapped, i.e. 200-byte remote writes over xGMI -- and the solve
 *                        kernel of each device waits for the world's posts in its own inbox and adds them in rank order
 *                        (bitwise identical everywhere); nothing is added to the streams.  Without peer access between
 *                        the devices the inboxes collapse into one box in pinned host memory (PCIe; env OA_MAILBOX=host
 *                        forces that, OA_MAILBOX=device refuses the fallback).  A device whose post does not arrive
 *                        within OA_EXCHANGE_TIMEOUT_S (default 30 s) ends the loop with OA_E_RCCL on every device.
 * Returns OA_E_RCCL when RCCL is asked for and cannot be brought up. */
#define OA_EXCHANGE_AUTO   (-1)
#define OA_EXCHANGE_MAILBOX 0
#define OA_EXCHANGE_RCCL    1
int         oa_set_exchange(oa_ctx *ctx, int mode);
void        oa_destroy(oa_ctx *ctx);
/* Released device blocks are kept in a process-wide cache for the next upload of the same size (hipFree costs
 * ~135 us a call, hipMalloc of 100 MB more): at most 256 MiB or what the library has had allocated at once, whichever is
 * larger (so that a re-upload of the same geometry allocates nothing; env OA_DEV_CACHE_MB sets a fixed cap instead,
 * OA_DEV_CACHE=0 switches the cache off), and nothing at all once the last context has been destroyed.  This gives
 * the cached blocks back immediately. */
void        oa_release_cached_memory(void);
const char *oa_last_error(void);
const char *oa_version(void);
/* stream: the hipStream_t every later call enqueues on, used exactly as given -- NULL is HIP's legacy default
 * stream (torch.cuda.current_stream() unless the caller changed it); OA_STREAM_OWN = the context's private
 * non-blocking stream (the default after oa_create). */
#define OA_STREAM_OWN ((void *)(intptr_t)-1)
int         oa_set_stream(oa_ctx *ctx, void *stream);

/* Correspondence-search strategy.  Every mode returns the same (index, d2) per source point, bit for bit:
 *   OA_SEARCH_BRUTE  k_nn_search_sorted: LDS-tiled brute force over all target vertices (the north-star kernel); its images of
 *                    the target, in the order of the longest axis, are built with the upload when this mode is set, else by
 *                    the call that sets it (a target uploaded for the other modes does not pay for them)
 *   OA_SEARCH_GRID   k_nn_search_grid: exact search through a uniform grid; points it cannot settle within a few
 *                    rings (far from the target: partial overlaps, holes) are finished by the tree search
 *   OA_SEARCH_BVH    k_bvh_search: every query through the 64-ary bounding-box tree, one wavefront per query
 *   OA_SEARCH_AUTO   the tree for small shards (up to ~1.2e4 .. 4e4 points, by target size and kind), the grid with
 *                    the tree behind it for larger ones; shards of up to ~1.4e4 .. 3.9e5 points take the tree while the
 *                    pose still moves and the grid once it has settled (decided on the device, per iteration);
 *                    brute force only for targets with non-finite coordinates
 * The same modes apply to surface targets (oa_set_target_mesh) with triangles in place of vertices.
 * Default: OA_SEARCH_AUTO (env OA_NN_GRID = 0 / 1 / 2 overrides at oa_create). */
#define OA_SEARCH_AUTO  (-1)
#define OA_SEARCH_BRUTE 0
#define OA_SEARCH_GRID  1
#define OA_SEARCH_BVH   2
int oa_set_search_mode(oa_ctx *ctx, int mode);

/* ---- one-time uploads (replaces BVHTree.FromObject, operators/icp_align.py:53, and the vlist
 *      walk over align_obj.data.vertices, functions/general.py:280-284) ------------------------ */
/* target (base object) vertices, base-LOCAL, n x 3 float32.  on_device != 0: xyz is a device pointer. */
int oa_set_target(oa_ctx *ctx, const float *xyz, int64_t n, int on_device);
/* SURFACE mode (the BVHTree.find_nearest semantics of functions/general.py:297): the base object's vertices plus
 * its triangles (n_tris x 3 vertex indices, host int32; quads/ngons triangulated by the caller, e.g. Blender's
 * loop_triangles).  The correspondence of a source point is then the closest point on the nearest triangle
 * (Ericson's closest-point-on-triangle in float32, lowest triangle index on ties) instead of the nearest vertex;
 * everything else (threshold, pair mapping, solve, loop) is unchanged.  oa_set_target() returns to vertex mode. */
int oa_set_target_mesh(oa_ctx *ctx, const float *xyz, int64_t n_verts, int on_device,
                       const int32_t *tris, int64_t n_tris);
/* source (align object) vertices, align-LOCAL, n_verts x 3 float32.
 * vlist (host, may be NULL = all vertices) is the operator's vertex list; stride > 1 applies
 * vlist[0::stride] (functions/general.py:274-275).  The selected list is then cut into shard_count shards of
 * ceil(n_selected / shard_count) points and this context keeps shard shard_index.  With shard_count > 1 the
 * shards are equal ranges of the selection in MORTON order (every rank passes the same arrays and derives the
 * same partition), so that a shard is a compact region of space; for non-finite coordinates they are contiguous
 * ranges in the caller's order.  Per-point outputs of a shard (oa_make_pairs, oa_nn_search) list its points in the
 * caller's order.  The sums the loop all-reduces do not depend on the partition.
 * On an oa_create_multi context pass shard 0 of 1: the context deals the shards to its devices itself.
 * Limits: a shard holds at most 65 535 x 256 x R selected points for the brute-force search (R = 4 points per
 * thread for shards >= 65 536 points: ~6.7e7; OA_NN_R=8 doubles it) -- beyond that oa_run fails with OA_E_BAD_ARG and
 * the job needs more shards; the grid / tree searches take any shard that fits an int32 (< 2^31 - 2^20 points).
 * Targets: < 2^31 - 2^16 vertices, < 7.1e8 triangles. */
int oa_set_source(oa_ctx *ctx, const float *xyz, int64_t n_verts, int on_device,
                  const int64_t *vlist, int64_t n_vlist, int32_t stride,
                  int32_t shard_index, int32_t shard_count);
/* EXTENSION (no counterpart in the reference): reject a pair when the angle between the world-space
 * normals of the source vertex and of its correspondence exceeds max_angle_deg.  src_normals: n_verts x 3 (align-
 * local, host); tgt_normals: nt x 3 per target vertex (vertex mode; ignored in surface mode, where the geometric
 * normal of the nearest triangle is used; NULL in vertex mode: the normals the target already has -- oa_set_target_normals,
 * oa_estimate_target_normals(install) -- stay in force, OA_E_BAD_ARG when it has none).  Call after oa_set_source / oa_set_target; passing src_normals == NULL
 * or an angle outside (0, 180) switches the test off; a new source or target upload switches it off too. */
int oa_set_normals(oa_ctx *ctx, const float *src_normals, int64_t n_verts, const float *tgt_normals, int64_t nt,
                   double max_angle_deg);
/* EXTENSION (no counterpart in the reference's code; its citation.txt names Chen & Medioni next to Besl & McKay): what a loop
 * step minimises.
 *   OA_METRIC_POINT  the distance of every source point to its correspondence (Besl-McKay; pairs -> Kabsch / SVD): the
 *                    reference's loop and the default
 *   OA_METRIC_PLANE  the distance of every source point to the TANGENT PLANE at its correspondence (Chen-Medioni): per pair
 *                    the residual n . (a - b) and the row [a x n, n] of the linearised step (omega, t) about the context's pivot
 *                    (oa_get_pivot), n = the correspondence's normal carried to align-local space -- the nearest triangle's
 *                    geometric normal (surface mode) or the target vertex normal (vertex mode: oa_set_target_normals or
 *                    oa_set_normals).  The 6 x 6 normal equations are solved through their eigen-decomposition; eigenvalues
 *                    below 1e-10 of the largest count as zero and the step is the minimum-norm one (a plane, a sphere, a
 *                    cylinder leave directions the data cannot see: the step does not move along them); the rotation is
 *                    exp([omega]x), exact.  Pairs are tested as for the point metric (thresh, normal-angle test); a pair whose
 *                    normal has zero or non-finite length takes no part in the step and is not counted in K.  Everything after
 *                    the step's matrix -- float32 new_mat, matrix_world @ new_mat, the convergence rings, history, report -- is
 *                    the point metric's code.  Every search mode serves it.
 * The metric survives uploads and oa_set_matrices; changing it ends a running oa_iterate sequence (the next call starts a new
 * one from the current matrix_world).  Under OA_METRIC_PLANE:
 *   - oa_run / oa_iterate with with_scale != 0 return OA_E_BAD_ARG (the step is rigid); with a vertex-mode target that has no
 *     normals OA_E_STATE; with a shard of more than 8 388 608 points OA_E_CAPACITY;
 *   - multi-device contexts (oa_create_multi) and the split-phase calls (oa_run_begin, oa_iter_partial, oa_iter_finish) return
 *     OA_E_STATE: their exchange carries OA_NSUMS doubles, the plane system needs 32;
 *   - oa_make_pairs, oa_nn_search, oa_kabsch* do not look at the metric. */
#define OA_METRIC_POINT 0   /* default: Besl-McKay, today's loop */
#define OA_METRIC_PLANE 1   /* Chen-Medioni */
#define OA_METRIC_GICP  2   /* plane-to-plane (Generalized-ICP: Segal, Haehnel, Thrun 2009), see oa_set_gicp */
#define OA_METRIC_SYMMETRIC 3   /* symmetric point-to-plane (Rusinkiewicz 2019): the rotation split between both sides, see below */
int oa_set_metric(oa_ctx *ctx, int metric);
/* OA_METRIC_GICP: every pair is weighted by a 3 x 3 matrix built from the local surface of BOTH sides.  For a
 * pair that passes the point metric's tests (thresh, the normal-angle test when it is on), with a', b' the pair about the
 * context's pivot, n_b the correspondence's unit normal in align-local space (exactly the plane metric's: the nearest triangle's
 * geometric normal, or the target vertex normal) and n_a the source vertex's normal (oa_set_source_normals / oa_set_normals:
 * align-local float32, normalised in fp64 the way n_b is: n * (1 / sqrt((x x + y y) + z z))):
 *   M = 2 I - (1 - epsilon)(n_a n_a^T + n_b n_b^T)    the sum of the paper's regularised covariances (eigenvalues 1, 1, epsilon)
 *   W = 2 epsilon M^-1                                  symmetric, fp64, adjugate over determinant (one division)
 *   e = a' - b',   J = [ -[a']x , I3 ],   step x = (omega, t):   minimise sum w (e + J x)^T W (e + J x)
 * The factor 2 epsilon does not move the step; with it e^T W e -> (n . e)^2 for n_a = n_b as epsilon -> 0, so residuals are in
 * the plane metric's units, and W = n n^T would give the plane metric's row exactly.  Normals that agree make a point-to-plane
 * pair; normals that disagree (an edge, a wrong correspondence, the rim of an overlap) leave a weak point-to-point pull.  Only
 * n n^T enters: the SIGNS of the normals drop out.  epsilon = 1 gives W = I, the Gauss-Newton point-to-point step.
 * A pair whose n_a or n_b has zero or non-finite length takes no part in the step and is not counted in K.  The normal
 * equations have the plane metric's shape: the same 32-double row, 6 x 6 minimum-norm solve (OA_STAT_PLANE_RANK) and code
 * after the step's matrix.  Pair weights (oa_set_robust with a fixed scale, oa_set_source_weights) take the residual
 * s sqrt(e^T W e), s as under OA_METRIC_PLANE.  Under OA_METRIC_GICP, when a loop starts:
 *   - with_scale != 0: OA_E_BAD_ARG; a shard of more than 8 388 608 points: OA_E_CAPACITY;
 *   - a vertex-mode target without normals, or a source without normals: OA_E_STATE;
 *   - oa_set_robust_auto switched on together with a loss: OA_E_STATE (the scale's selection knows the other two metrics only);
 *   - multi-device contexts and the split-phase calls: OA_E_STATE, as under OA_METRIC_PLANE.
 * Each refusal leaves the context usable.  oa_make_pairs, oa_nn_search, oa_kabsch*, oa_point_to_plane, oa_coarse_align do not
 * look at the metric.
 * oa_set_gicp: epsilon must be finite and in [1e-6, 1], else OA_E_BAD_ARG; default 1e-3 (the paper's).  It survives uploads and
 * oa_set_matrices; changing it ends a running oa_iterate sequence, as oa_set_metric does. */
int oa_set_gicp(oa_ctx *ctx, double epsilon);
/* OA_METRIC_SYMMETRIC: the symmetric objective (Rusinkiewicz, "A Symmetric Objective Function for ICP", SIGGRAPH 2019;
 * DESIGN.md 3.20).  It uses the two normals of OA_METRIC_GICP, has no parameter, and its row is rank one: the plane metric's
 * 32-double row, 6 x 6 minimum-norm solve (OA_STAT_PLANE_RANK) and everything after the step's matrix serve it.  A pair takes
 * part if it passes the point metric's tests (thresh, the normal-angle test when it is on, the reciprocal / trim verdict).  With
 * a', b' the pair about the context's pivot exactly as under OA_METRIC_PLANE, n_b the correspondence's unit normal exactly as
 * under OA_METRIC_PLANE, and n_a the source vertex's normal normalised as under OA_METRIC_GICP (n * (1 / sqrt((x x + y y) + z z));
 * a source normal of zero or non-finite length drops the pair from the step and from K):
 *   s = (n_a . n_b < 0) ? -1 : +1                 (left-to-right sum; an exact 0 counts as +1)
 *   n = (n_b + s n_a) / 2                         |n|^2 = (1 + |cos|) / 2 in [1/2, 1]: never zero, never dropped
 *   r = n . (a' - b'),   J = [ (a' + b') x n , n ],   step x = (a~, t~) minimises sum w (r + J . x)^2
 *   theta = atan(|a~|),  R = exp(theta [a~ / |a~|]x),  t = t~ cos(theta)          (|a~| = 0: R = I, t = t~)
 *   M = T(c) R T(t) R T(-c)                       c the pivot: half the rotation before the translation, half after
 *   - r is exactly zero for a pair on a patch of constant curvature, whatever the rotation between the two sides; the plane
 *     metric's error is first order in that rotation.
 *   - Flipping the sign of any n_a leaves n the same bits.  Flipping any n_b flips n, J and r together, so every term of
 *     sum J J^T and sum J r keeps its bits: the signs of estimated, unoriented normals do not matter.
 *   - For agreeing normals |n| = 1 and r is the plane metric's distance in the plane metric's units: res_scale, oa_set_robust's
 *     scale and the sum of r^2 mean what they mean under OA_METRIC_PLANE.  Weighted: w = w_vertex psi(res_scale |r|).
 *   - oa_set_trim (fixed and estimated share) and oa_set_robust_auto work under this metric, on the key res_scale |r|.
 * Under OA_METRIC_SYMMETRIC, when a loop starts: with_scale != 0: OA_E_BAD_ARG; a vertex-mode target without normals, or a
 * source without normals (oa_set_source_normals / oa_set_normals): OA_E_STATE; a shard of more than 8 388 608 points:
 * OA_E_CAPACITY; multi-device contexts and the split-phase calls: OA_E_STATE, as under OA_METRIC_PLANE.  Each refusal leaves the
 * context usable.  OA_STAT_ACC_PATH reports OA_ACC_PLANE (the plane kernel's row and epilogue).  oa_make_pairs, oa_nn_search,
 * oa_kabsch*, oa_point_to_plane, oa_symmetric_step, oa_coarse_align do not look at the metric. */
/* per-vertex source normals (align-local, n_verts x 3 float32, host; n_verts as given to oa_set_source) for OA_METRIC_GICP,
 * without switching the normal-angle test on: the counterpart of oa_set_target_normals.  The array is the one oa_set_normals
 * fills and the normal-angle test reads -- either call overwrites it, switching the test off keeps it, a new source upload
 * forgets it.  Call after oa_set_source (OA_E_STATE otherwise); a wrong n_verts is OA_E_BAD_ARG.  Ends a running oa_iterate
 * sequence, as oa_set_target_normals does.  Multi-device contexts route it to every child. */
int oa_set_source_normals(oa_ctx *ctx, const float *src_normals, int64_t n_verts);
/* vertex-mode targets: per-vertex normals (base-local, nt x 3 float32, host) for the plane metric, without switching the
 * normal-angle test on; a new target upload forgets them.  Normals given through oa_set_normals serve as well. */
int oa_set_target_normals(oa_ctx *ctx, const float *tgt_normals, int64_t nt);
/* EXTENSION: normals for a point-cloud target, estimated on the device -- a raw scan has none to bring.
 *
 * oa_target_knn: vertex-mode targets.  For every target vertex i, its k nearest target vertices (itself included) in the
 * library's exact order: ascending (d2_metric(v_i, v_j), j), lowest index first on ties.  Outputs in the caller's vertex order
 * and indexing, row-major nt x k, host memory; either may be NULL.  Coordinates are the target's own (base-local), no matrices
 * needed.  1 <= k <= min(64, nt), else OA_E_BAD_ARG; OA_E_STATE without a target and for a surface target.  A vertex with a
 * non-finite coordinate has no finite distance to anything: its row is empty (index -1, d2 +inf) and it is in nobody's row; a row
 * with fewer than k finite distances is padded the same way.  The search walks the target's box tree; a context that has none
 * (OA_SEARCH_BRUTE, non-finite coordinates) builds one for the call. */
int oa_target_knn(oa_ctx *ctx, int k, int32_t *out_idx, float *out_d2);

#define OA_ORIENT_NONE   0   /* canonical sign: the component of largest magnitude is positive (lowest axis on equal magnitude) */
#define OA_ORIENT_TOWARD 1   /* n . (orient_point - v) >= 0   (a scanner position) */
#define OA_ORIENT_AWAY   2   /* n . (v - orient_point) >= 0   (an interior point; NULL orient_point = the target's fp64 centroid) */
/* PCA normals from each vertex's k nearest neighbours (oa_target_knn's rows): unit eigenvector of the smallest eigenvalue of the
 * neighbourhood's covariance, float32, base-local (what oa_set_target_normals takes); curvature = l0 / (l0 + l1 + l2) ("surface
 * variation").  The covariance is fp64 and two-pass (the mean of the k points, then centred products, both summed in list
 * order), the eigen-solve a cyclic Jacobi in fp64, the vector normalised in fp64 and rounded once; no atomics: two calls give
 * the same bits.  The sign is the canonical one, then flipped where the orientation rule asks for it (evaluated in fp64).
 * Degenerate neighbourhoods -- with l0 <= l1 <= l2: l1 <= 1e-12 l2, l2 zero or not finite (collinear or identical points), or
 * fewer than three neighbours at a finite distance (non-finite coordinates) -- get the normal (0, 0, 0) and curvature 0; the
 * plane metric drops pairs with a zero normal and does not count them in K.
 * install != 0: the result becomes the context's target normals on the device, as after oa_set_target_normals, without a host
 * round trip; a new target upload forgets them.  out_normals (nt x 3) / out_curvature (nt) may be NULL.
 * 3 <= k <= min(64, nt) and orient in 0 .. 2, else OA_E_BAD_ARG; OA_ORIENT_TOWARD with a NULL point OA_E_BAD_ARG; OA_E_STATE
 * without a target and for a surface target (oa_set_target_mesh: it uses its triangles' normals).
 * Both calls end a running oa_iterate sequence, as oa_set_target_normals does.  Multi-device contexts route them to every child
 * (the target is replicated: the same bits everywhere); the host outputs are the first child's. */
int oa_estimate_target_normals(oa_ctx *ctx, int k, int orient, const float orient_point[3], int install,
                               float *out_normals, float *out_curvature);
/* EXTENSION: one consistent sign for the normals of a point-cloud target -- Hoppe, DeRose, Duchamp, McDonald &
 * Stuetzle 1992: signs handed along the minimum spanning forest of the neighbour graph.  The orient rules above point every normal
 * at or away from ONE point, which is right only for a star-shaped object seen from there; this call needs no such point.
 * Vertex-mode targets, single-device contexts.
 * Normals: `normals` (nt x 3, host), or with NULL the context's own (OA_E_STATE when it has none).  A vertex is ELIGIBLE when its
 * normal is finite and not (0, 0, 0) and its coordinates are finite; every other vertex is left out: its normal comes back as it
 * was, flipped 0, component -1, counted in n_left_out.
 * Graph: with the rows of oa_target_knn(k), an undirected edge {i, j}, i != j, when j is in row(i) or i is in row(j), both ends
 * are eligible and, with max_dist > 0, the row's d2 <= (float)max_dist * (float)max_dist (float32; max_dist = 0: no cap).
 * Weight and flip, float32 with one rounding per operation: d = (nx_i nx_j + ny_i ny_j) + nz_i nz_j; t = 1 - |d|;
 * w = t > 0 ? t : 0; the edge flips iff d < 0.
 * Tree: the minimum spanning forest under the strict total order (w, min(i, j), max(i, j)), indices in the caller's order: it is
 * unique.  Within a component the sign of v relative to u is the product of the flips on the tree path between them.
 * Seed: per component one vertex decides the overall sign --
 *   OA_SEED_KEEP    the lowest index; it keeps the sign it came with
 *   OA_SEED_TOWARD  the vertex nearest to point:    n . (point - v) >= 0
 *   OA_SEED_AWAY    the vertex farthest from point: n . (v - point) >= 0; a NULL point is the target's fp64 centroid
 * nearest / farthest by the fp64 squared distance (dx dx + dy dy) + dz dz, d = (double)v - (double)point, the lowest index on
 * ties; the sign test is the fp64 dot product (x x + y y) + z z, and a dot of exactly 0 keeps the sign.
 * Outputs (host, each may be NULL): out_normals = the normals with the sign bit of all three components toggled or not -- no
 * renormalisation, so given the rows the result is exact; out_flipped 0 / 1; out_component = the lowest index of the vertex's
 * component.  rep: the number of components, of vertices left out and of vertices flipped, and the merging rounds that ran.
 * install != 0: the result becomes the context's target normals on the device, as after oa_estimate_target_normals with install
 * (in place, without a host round trip, when they were the input).  Integer atomics and comparisons only: two calls give the
 * same bits.  The call ends a running oa_iterate sequence, as oa_estimate_target_normals does.
 * OA_E_BAD_ARG: k outside 2 .. min(64, nt); seed outside 0 .. 2; OA_SEED_TOWARD with a NULL point; a non-finite point; max_dist
 * negative or not finite.  OA_E_STATE: no target, a surface target, a multi-device context, NULL normals and none installed.
 * OA_E_CAPACITY: nt k > 2^31 - 2^20.  OA_E_HIP should a round's bound be exceeded (never seen).  Each refusal leaves the context usable. */
typedef struct oa_orient_report {
    int64_t n_components;           /* components of the graph over the eligible vertices */
    int64_t n_left_out;             /* vertices that are not eligible */
    int64_t n_flipped;              /* vertices whose normal changed sign */
    int32_t rounds, reserved;       /* Boruvka rounds in which components merged */
} oa_orient_report;
#define OA_SEED_KEEP   0   /* each component's lowest-index vertex keeps the sign it came with */
#define OA_SEED_TOWARD 1   /* each component's vertex NEAREST to point: n . (point - v) >= 0   (a scanner position) */
#define OA_SEED_AWAY   2   /* each component's vertex FARTHEST from point: n . (v - point) >= 0; NULL point = the target's fp64 centroid */
int oa_orient_target_normals(oa_ctx *ctx, int k, double max_dist, int seed, const float point[3],
                             const float *normals /* nt x 3 host, or NULL: the context's target normals */, int install,
                             float *out_normals /* nt x 3 */, uint8_t *out_flipped /* nt */, int32_t *out_component /* nt */,
                             oa_orient_report *rep);
/* EXTENSION: stray points of a point-cloud target -- flying pixels, dust, the scanner table.  Vertex-mode targets,
 * single-device contexts.  Coordinates are the target's own (base-local), no matrices needed.
 *
 * oa_target_radius_count: count[i] = min(cap, #{ j : d2_metric(v_i, v_j) <= r2 }), r2 = (float)radius * (float)radius (float32, one
 * rounding; the rule of oa_orient_target_normals' max_dist), in the caller's vertex order.  The vertex itself is included, so a
 * finite vertex counts at least 1, and duplicates count.  cap = 0: no cap; else the count saturates at cap (the search of that
 * vertex stops there; the value does not depend on the order of the search).  A vertex with a non-finite coordinate counts 0
 * and is counted by nobody.  Exact: every hit is one evaluation of the float32 metric, and a pair at d2 = r2 is never lost.
 *
 * oa_target_outliers: a keep mask for the resident target and, with apply != 0, the target without the others.
 *   OA_OUTLIER_STATISTICAL  score[i] = the mean distance from vertex i to its k nearest OTHER vertices: with the k + 1 entries of
 *       oa_target_knn's row, S = sum over the m filled entries of sqrt((double)d2), in list order, fp64; score = S / (m - 1), +inf
 *       for m < 2 (a non-finite vertex).  The vertex itself contributes 0.  n = the number of finite scores, mean = sum / n,
 *       std = sqrt(sum (score - mean)^2 / (n - 1)) (two passes; 0 for n < 2), both fp64 in a fixed order without floating-point
 *       atomics: two calls give the same bits.  threshold = mean + std_ratio std; keep[i] = score[i] <= threshold.
 *   OA_OUTLIER_RADIUS       count[i] = oa_target_radius_count(radius, count_cap); keep[i] = count[i] - 1 >= min_neighbors.
 * Outputs (host, each may be NULL): keep (nt bytes, 0 / 1); score (nt, STATISTICAL) or count (nt, RADIUS) -- the other is not
 * written; kept_index = the kept vertices in ascending order (n_kept entries; give room for nt); rep.
 * apply != 0: the resident target becomes the kept vertices in the caller's order, compacted on the device and taken the way
 * oa_set_target(..., on_device = 1) takes them -- grid, tree and sorted images rebuilt, seeds reset, installed normals, descriptors
 * and boundary masks forgotten: the context is what oa_set_target(xyz[keep]) would have left.  OA_STAT_TARGET_CLEANED then holds
 * the number of vertices removed.  When no vertex would be kept: OA_E_TOO_FEW_PAIRS, nothing applied, the outputs written.
 * Both calls end a running oa_iterate sequence, as oa_target_knn does; a context without a box tree builds one for the call.
 * OA_E_BAD_ARG: an unknown method; the ranges beside the fields below; a radius that is not finite and > 0; cap < 0.
 * OA_E_STATE: no target, a surface target, a multi-device context.  Each refusal leaves the context usable. */
#define OA_OUTLIER_STATISTICAL 0
#define OA_OUTLIER_RADIUS      1
typedef struct oa_outlier_settings {
    int32_t method, k;            /* STATISTICAL: 1 <= k <= min(63, nt - 1) */
    double  std_ratio;            /* STATISTICAL: finite, >= 0 */
    double  radius;               /* RADIUS: finite, > 0, the target's own (base-local) units */
    int32_t min_neighbors;        /* RADIUS: >= 1; neighbours = count - 1 */
    int32_t count_cap;            /* RADIUS: 0 = exact counts, else >= min_neighbors + 1: counts saturate there */
} oa_outlier_settings;
typedef struct oa_outlier_report {
    int64_t n_kept, n_removed, n_nonfinite;   /* n_nonfinite: vertices with a non-finite coordinate (never kept) */
    double  mean, std, threshold; /* STATISTICAL; 0 for RADIUS */
} oa_outlier_report;
int oa_target_outliers(oa_ctx *ctx, const oa_outlier_settings *s, int apply,
                       uint8_t *keep /* nt */, double *score /* nt, STATISTICAL */, int32_t *count /* nt, RADIUS */,
                       int32_t *kept_index /* n_kept entries, room for nt */, oa_outlier_report *rep);
int oa_target_radius_count(oa_ctx *ctx, double radius, int32_t cap, int32_t *count /* nt */);
/* EXTENSION: radius-limited neighbourhoods.  The k nearest vertices reach as far as it takes: across a thin wall
 * scanned from both sides, to the next tooth, over a hole narrower than their spread.  With a neighbour radius set, the rows of
 * oa_target_knn are "the k nearest among the vertices with d2_metric(v_i, v_j) <= r2", r2 = radius * radius in float32 (one
 * rounding; the constant oa_target_radius_count(radius) compares against): ascending (d2, index) as before, d2 = r2 included,
 * shorter rows padded with -1 / +inf as rows of a target with non-finite vertices already are.  Exact: a vertex beyond r2 never
 * enters a list and a box is skipped only when everything inside is strictly beyond min(k-th best, r2).
 * The setting limits oa_target_knn, oa_estimate_target_normals (fewer than 3 neighbours: the zero normal), oa_target_fpfh (an
 * unfilled entry takes no part) and the cloud criterion of oa_target_boundary / oa_set_reject_boundary (fewer than 3 usable
 * neighbours: on the boundary; a mask built under another radius is rebuilt).  oa_orient_target_normals has its own max_dist and
 * does not look at it; oa_target_outliers, oa_target_radius_count, oa_target_clusters and oa_target_spacing neither.
 * radius: 0 = no limit (the default: every byte of every call is what it was without the setting); else finite, > 0, in the
 * target's own (base-local) units, with a finite float32 square -- anything else is OA_E_BAD_ARG and changes nothing.  A setting
 * like the metric: it survives uploads and oa_set_matrices, multi-device contexts hand it to every child, a change ends a running
 * oa_iterate sequence, and it costs nothing until one of the four calls runs.  oa_get_neighbor_radius reads the float32 back. */
int oa_set_neighbor_radius(oa_ctx *ctx, float radius);
int oa_get_neighbor_radius(oa_ctx *ctx, float *radius);
/* The cloud's own point spacing -- the scale a neighbour radius, a voxel edge or an eps is a multiple of.  Vertex-mode targets,
 * single-device contexts.  s[i] = the distance from vertex i to the nearest OTHER vertex: oa_target_outliers' STATISTICAL score at
 * k = 1, sqrt((double)d2) of entry 1 of oa_target_knn's row (a duplicate gives 0; the neighbour radius does not apply).  mean and std
 * over the finite s[i] by that filter's fixed-order fp64 passes (std = sqrt(sum (s - mean)^2 / (n - 1)), 0 for n < 2): two calls
 * give the same bits.  n_finite = the vertices with a finite s[i]; n_nonfinite = nt - n_finite: those with a non-finite
 * coordinate (and a vertex that is the only finite one of its cloud).  Without a finite s[i] mean and std are 0.
 * OA_E_BAD_ARG for a NULL argument; OA_E_STATE: no target, a surface target, a multi-device context.  Ends a running oa_iterate
 * sequence, as oa_target_radius_count does.  Each refusal leaves the context usable. */
typedef struct oa_spacing_report {
    double  mean, std;
    int64_t n_finite, n_nonfinite;
} oa_spacing_report;
int oa_target_spacing(oa_ctx *ctx, oa_spacing_report *rep);
/* EXTENSION: the parts of a point-cloud target -- DBSCAN labels, and the target without the scanner table, the
 * clamp or a second object, which the filters above cannot remove because such parts are dense.  Vertex-mode targets,
 * single-device contexts.  Coordinates are the target's own (base-local), no matrices needed.
 *
 * The contract, with r2 = (float)eps * (float)eps (float32, one rounding; oa_target_radius_count's rule) and d2_metric the float32
 * metric of the searches, has exactly one answer:
 *   count[i] = #{ j : d2_metric(v_i, v_j) <= r2 }; the vertex itself is included, duplicates count; a vertex with a non-finite
 *       coordinate counts 0 and is counted by nobody.  core[i] = count[i] >= min_points.
 *   Two core vertices are linked iff d2_metric <= r2.  d2_metric is symmetric bit for bit, so the graph is undirected.  A cluster
 *       is a connected component of the core graph; clusters are numbered 0, 1, ... in ascending order of their lowest core index.
 *   A non-core vertex with at least one core vertex within the radius is a border vertex: its label is the lowest label among the
 *       clusters of those core vertices.  Everything else is noise, label -1.
 *   sizes[c] = the core and border members of cluster c.  The largest cluster is the one of greatest size, on equal size the lowest label.
 * This is what scikit-learn's DBSCAN(algorithm="brute") returns, numbering and border assignment included.  Integer atomics and
 * comparisons only: two calls give the same bits, whichever order the device ran its waves in.
 * keep[i]: OA_CLUSTER_KEEP_CLUSTERED label >= 0; _LARGEST label = the largest cluster's; _MIN_SIZE label >= 0 and sizes[label] >= min_size.
 * Outputs (host, each may be NULL): label (nt); sizes (n_clusters entries; give room for nt); keep (nt bytes, 0 / 1); kept_index =
 * the kept vertices in ascending order (n_kept entries; give room for nt); rep.
 * apply != 0: as oa_target_outliers -- the resident target becomes the kept vertices in the caller's order, the context is what
 * oa_set_target(xyz[keep]) would have left, OA_STAT_TARGET_CLEANED holds the number removed.  When no vertex would be kept:
 * OA_E_TOO_FEW_PAIRS, nothing applied, the outputs written.
 * The call ends a running oa_iterate sequence, as oa_target_knn does; a context without a box tree builds one for the call.
 * OA_E_BAD_ARG (decided before any launch): NULL settings; eps not finite or not > 0; min_points < 1; an unknown keep; min_size < 0.
 * OA_E_STATE: no target, a surface target, a multi-device context.  OA_E_HIP should the union-find's step bound be exceeded (never
 * seen).  Each refusal leaves the context usable. */
#define OA_CLUSTER_KEEP_CLUSTERED 0   /* label >= 0: the noise goes */
#define OA_CLUSTER_KEEP_LARGEST   1
#define OA_CLUSTER_KEEP_MIN_SIZE  2   /* sizes[label] >= min_size */
typedef struct oa_cluster_settings {
    double  eps;                  /* finite, > 0, the target's own (base-local) units */
    int32_t min_points, keep;     /* min_points >= 1 (1: plain Euclidean clustering); keep: OA_CLUSTER_KEEP_* */
    int64_t min_size;             /* >= 0; read by OA_CLUSTER_KEEP_MIN_SIZE alone */
} oa_cluster_settings;
typedef struct oa_cluster_report {
    int64_t n_clusters, n_core, n_border;
    int64_t n_noise, n_nonfinite; /* n_noise: every vertex of label -1, the n_nonfinite vertices with a non-finite coordinate among them */
    int64_t largest_label, largest_size;      /* -1, 0 without a cluster */
    int64_t n_kept, n_removed;
} oa_cluster_report;
int oa_target_clusters(oa_ctx *ctx, const oa_cluster_settings *s, int apply,
                       int32_t *label /* nt */, int32_t *sizes /* n_clusters entries, room for nt */,
                       uint8_t *keep /* nt */, int32_t *kept_index /* n_kept entries, room for nt */, oa_cluster_report *rep);
/* EXTENSION (no counterpart in the reference, whose only protection against bad correspondences is the hard cut thresh): pair
 * weights.  Every pair of a loop step (oa_run, oa_iterate, the split-phase calls) carries the weight
 *   w = w_vertex * psi(r),   c = scale (world units, like thresh):
 *   OA_LOSS_NONE    psi = 1 (default)
 *   OA_LOSS_HUBER   psi = 1 for r <= c, else c / r
 *   OA_LOSS_TUKEY   psi = (1 - (r/c)^2)^2 for r < c, else 0
 *   OA_LOSS_CAUCHY  psi = 1 / (1 + (r/c)^2)
 * (fixed scale, an iteratively re-weighted step; all three continuous in r).  The residual r is
 *   OA_METRIC_POINT  the world-space pair distance the thresh test measures;
 *   OA_METRIC_PLANE  s |n . (a - b)|, the distance to the tangent plane, s = cbrt(|det(mx_align[:3,:3])|) carrying the
 *                    align-local residual to world units (taken when the loop starts; the plane step is rigid).
 * Point metric: the sums of a, b, b a^T, |a|^2, |b|^2 are weighted and slot 20 of the OA_NSUMS row holds sum w, from which the
 * solve takes its mass (centroids, covariance, scale); plane metric: sum J J^T and sum J r are weighted.  K (oa_report.last_K,
 * stats[0]) stays the COUNT of pairs -- a pair of weight 0 is counted -- and mean_dist / std_dist stay unweighted.  A step fails
 * with OA_E_TOO_FEW_PAIRS when K < 3, as ever, and when sum w is not > 0.
 * With OA_LOSS_NONE and no vertex weights nothing changes: the same kernels, the same bits, slot 20 = 0.  Otherwise the loop
 * runs search -> accumulate (no accumulating search epilogue) and takes shards of up to 8 388 608 points (OA_E_CAPACITY).
 * The weighted point metric runs on every kind of context -- single-device, oa_create_multi (mailbox and RCCL), oa_run_begin /
 * oa_iter_partial / oa_iter_finish: the row is still OA_NSUMS doubles; the weighted plane metric on single-device contexts, as
 * the plane metric itself.  oa_make_pairs, oa_nn_search, oa_kabsch*, oa_point_to_plane do not look at the loss or the weights
 * (oa_kabsch_from_sums ignores slot 20).
 * oa_set_robust: OA_E_BAD_ARG for an unknown loss, and for a loss other than NONE with a scale that is not finite and > 0.  The
 * setting survives uploads and oa_set_matrices; changing it ends a running oa_iterate sequence, as oa_set_metric does. */
#define OA_LOSS_NONE   0
#define OA_LOSS_HUBER  1
#define OA_LOSS_TUKEY  2
#define OA_LOSS_CAUCHY 3
int oa_set_robust(oa_ctx *ctx, int loss, double scale);
/* EXTENSION: the loss's scale from each step's own residuals instead of a fixed one -- residuals are centimetres when an
 * alignment starts and tens of microns when it ends, and no fixed c suits both.  With quantile p in (0, 1] and a floor
 * scale_min (world units, finite and > 0), step i uses
 *   c_i = max(m * q_i, scale_min),   m = the `scale` of oa_set_robust, now a dimensionless multiplier,
 *   q_i = the k-th smallest, k = ceil(p * K_q) (1-based, fp64), of the float32-rounded residuals r of THIS step's pairs at THIS
 *         step's pose -- the r the loss is applied to (see oa_set_robust) -- over the K_q pairs that are counted in K and carry
 *         a vertex weight > 0 (zero/one vertex weights stay a vlist); a plain order statistic: no interpolation, no weighting.
 *         K_q = 0: c_i = scale_min.  c_i is formed in fp64 from (double)q_i.
 * p = 0.5 with m = 1.4826 x the loss's usual tuning constant is the median-absolute-deviation scale ("tukey" and nothing else
 * to tune).  The selection is exact and runs on the device between the search and the weighted accumulation (a radix select
 * over the residuals' bits, integer counts only: the same bits on every run), without a host round trip; nothing else about
 * the step changes, and OA_STAT_ROBUST_SCALE reads c_i back.
 * quantile == 0 switches it off (the default; scale_min is then ignored) and nothing changes: the same kernels, the same bits.
 * OA_E_BAD_ARG for a quantile outside [0, 1] and, with quantile > 0, a floor that is not finite and > 0.  With OA_LOSS_NONE the
 * setting is remembered and inert.  It survives uploads and oa_set_matrices; changing it ends a running oa_iterate sequence, as
 * oa_set_robust does.
 * Single-device contexts, oa_run / oa_iterate only: a quantile of the world's residuals needs the world's histogram, and the
 * exchange between devices carries OA_NSUMS doubles -- with the setting on and a loss set, oa_run / oa_iterate of a multi-device
 * context and oa_run_begin / oa_iter_partial fail with OA_E_STATE (the context stays usable; oa_set_robust_auto(ctx, 0, 0)
 * brings the fixed scale back). */
int oa_set_robust_auto(oa_ctx *ctx, double quantile, double scale_min);

/* EXTENSION (not in the reference; PCL's and libpointmatcher's reciprocal correspondence filter): keep a pair only if it is
 * mutual.  Every step pairs each selected source point with its nearest target point; with the check on, the opposite question
 * is asked too: is this source point also the nearest one to its correspondence?  Where the source reaches beyond the target
 * (a whole model against a partial scan, two partial scans) every source point outside the overlap pairs with the target's rim;
 * those pairs are not mutual, and with the check on they no longer drag the fit.
 *
 * Definition.  Slot i holds a pair when pair_eval accepts it: dist < thresh, and the normal-angle test when it is on.  Let
 * b = imx1 @ (mx2 @ co1) be the float32 point that make_pairs emits in B.  It is PairFetch::bx, by, bz, identical in vertex mode
 * and in surface mode.  Let p_k be the selected source points.  These are the packed src4 rows: the selection after vlist, stride
 * and sample_voxel.
 *   - d2(b, p) = d2_metric(b, p) is the project's fp32 difference form with its two fmas.  It is symmetric in its arguments.
 *   - m = min_k d2(b, p_k) over all selected slots.  A non-finite d2 never wins.
 *   - The pair is kept iff d2(b, p_i) <= r2 * m, with r2 = (float)(ratio * ratio) and one fp32 multiply.
 *   - With ratio = 1, the default, this reads "p_i is a nearest selected source point of its own correspondence".  Ties are
 *     kept.  The result does not depend on index order.
 *   - ratio lies in [1, 16]; anything else is OA_E_BAD_ARG.
 * A rejected pair takes no part in anything that pair_eval's verdict feeds: the sums of all three metrics, the weighted kernels,
 * the automatic robust scale's residuals, oa_make_pairs, and K, mean and std in the report.  oa_nn_search, oa_deviation,
 * oa_score_poses, and the scoring and refinement inside oa_coarse_align* do not apply the check: their results are the same bits
 * whether it is set or not.  The check is exact (a box tree over the selected source points in align-local space, built by the
 * first step after an oa_set_source and valid at every pose) and runs on the device between the search and the accumulation; a
 * step with the check on runs search -> check -> accumulate (no accumulating search epilogue).  Fewer than 3 surviving pairs is
 * OA_E_TOO_FEW_PAIRS, as ever; a source whose tree would need more than 6 levels OA_E_CAPACITY.  on == 0 (the default) changes
 * nothing: the same kernels, the same bits.  The setting survives uploads and oa_set_matrices; changing it ends a running
 * oa_iterate sequence, as oa_set_robust does.
 * Single-device contexts holding the whole selection, oa_run / oa_iterate / oa_make_pairs: a context that holds only a shard
 * cannot see the other shards' source points -- with the check on, loops and oa_make_pairs of a multi-device context,
 * oa_run_begin / oa_iter_partial, and any loop over a source uploaded with shard_count > 1 fail with OA_E_STATE (the context
 * stays usable; oa_set_reciprocal(ctx, 0, 1) brings the plain pairs back). */
int oa_set_reciprocal(oa_ctx *ctx, int on, double ratio);

/* EXTENSION (not in the reference; Trimmed ICP, Chetverikov et al. 2002/2005, and its fractional form, Phillips, Liu and Tomasi
 * 2007; PCL's CorrespondenceRejectorTrimmed, libpointmatcher's TrimmedDist / VarTrimmedDist filters): every step keeps only the
 * pairs with the smallest residuals.  The share kept is the overlap of the two clouds -- given (fraction in (0, 1]) or estimated
 * by every step itself (fraction = OA_TRIM_AUTO).  Unlike a robust loss it needs no scale in world units; unlike the reciprocal
 * check no tree over the source, and it drops displaced outliers as well as the rim of an overlap.
 *
 * Candidates.  The K_q pairs of a step that would be counted in K and carry a vertex weight > 0 (oa_set_robust_auto's
 * population; with oa_set_reciprocal on, the pairs that passed it).  Each has the float32-rounded residual r the losses use:
 * the world-space pair distance (point metric), s |n . (a - b)| (plane), s sqrt(e^T W e) (GICP).
 *   - Fixed share: k = clamp(ceil(fraction K_q), min(3, K_q), K_q) in fp64, 1-based; the cut q is the k-th smallest r.
 *   - Estimated share: with r_(1) <= ... <= r_(K_q), S_j = sum_{i <= j} (double)r_(i)^2 and J(j) = S_j j^-(1 + 2 lambda) (FICP's
 *     FRMSD^2 up to a factor without j): k = the smallest j in [k_min, K_q] that minimises J, k_min = clamp(ceil(fraction_min
 *     K_q), min(3, K_q), K_q); q = r_(k).  S_j is summed in fp64 in a fixed order (bitwise repeatable); against a sequential
 *     sum J differs by parts in 1e-10 at most, which can move k only between ranks whose J agree that closely.
 *   - A candidate stays iff r <= q, compared in float32: ties stay, at least k pairs stay, and nothing depends on slot order.
 *     A slot that is no candidate keeps the verdict it had (weight 0; a zero normal under the plane metrics).  K_q = 0: q = 0.
 * A trimmed pair is a rejected pair in oa_set_reciprocal's sense: it leaves the sums of all three metrics, the weighted kernels,
 * K, mean_dist / std_dist (so the convergence test runs on the trimmed statistics) and oa_set_robust_auto's population.  The step
 * runs search -> [reciprocal check] -> trim -> [robust scale] -> accumulate, never the accumulating search epilogue.
 * oa_make_pairs applies the trim with the point residual (it does not look at the metric); fewer than 3 surviving pairs is
 * OA_E_TOO_FEW_PAIRS.  oa_nn_search, oa_deviation, oa_score_poses and the coarse stages do not look at the setting.
 * Arguments: fraction = 0 (off, the default), a value in (0, 1], or OA_TRIM_AUTO; fraction_min in (0, 1] when the share is
 * estimated (ignored otherwise); lambda finite and in [0.5, 8] (2 is a sound default).  Anything else is OA_E_BAD_ARG and the
 * setting in force stays.  fraction = 0 changes nothing: the same launches, the same bits.  The setting survives uploads and
 * oa_set_matrices; changing it ends a running oa_iterate sequence.  The estimated share takes selections of up to 8 388 608
 * points (OA_E_CAPACITY beyond).
 * Single-device contexts holding the whole selection, oa_run / oa_iterate / oa_make_pairs: the cut is an order statistic of the
 * world's residuals -- with the trim on, loops and oa_make_pairs of a multi-device context, oa_run_begin / oa_iter_partial, and
 * any loop over a source uploaded with shard_count > 1 fail with OA_E_STATE (the context stays usable; oa_set_trim(ctx, 0, 0, 2)
 * brings the plain pairs back). */
#define OA_TRIM_AUTO (-1.0)
int oa_set_trim(oa_ctx *ctx, double fraction, double fraction_min, double lambda);

/* EXTENSION (not in the reference; Turk & Levoy 1994, Rusinkiewicz & Levoy 2001 "Efficient variants of ICP" 3.4): the target's
 * BOUNDARY, and the rejection of pairs whose correspondence lies on it.  Where the source reaches beyond a partial scan every
 * source point outside the overlap pairs with the scan's rim; the rim is a property of the target alone, found once.
 *
 * Mesh targets (oa_set_target_mesh): exact, integers only.
 *   - Local edge j of triangle t joins corners j and (j + 1) mod 3 (ab, bc, ca: the order of oa_deviation's edge features).
 *   - An undirected edge {u, v} with u != v is a boundary edge iff exactly one triangle, each triangle counted once, lists both
 *     u and v.  Edges with u == v are never boundary; edges shared by three or more triangles are not boundary.
 *   - A vertex is a boundary vertex iff it is an end of a boundary edge.
 *   - edge_mask[n_tris]: uint8, bit j = local edge j is a boundary edge.  vertex_mask[n_verts]: uint8, 0 or 1.
 *   - Coordinates play no part: zero-area triangles count like any other.
 * Point-cloud targets (oa_set_target): the angle criterion with parameters k and angle_deg.  The target's normals must be
 * installed (oa_set_target_normals, oa_set_normals, or an installed estimate), else OA_E_STATE.  For vertex i with float32
 * normal n, everything in fp64 on the float32 values:
 *   - Its neighbours are the first k entries of oa_target_knn's row of k + 1 whose index is not i.
 *   - The tangent basis is u = normalise(n x e) and v = n^ x u, e the coordinate axis of n's smallest-magnitude component
 *     (lowest axis on ties).
 *   - A neighbour whose tangent projection (d.u, d.v) is (0, 0) or not finite is skipped.
 *   - theta = atan2(d.v, d.u), sorted ascending; the gaps are the consecutive differences plus the wrap-around gap
 *     (theta_0 + 2 pi - theta_last).  The vertex is flagged iff the largest gap is greater than angle_deg pi / 180.
 *   - A vertex with a zero or non-finite normal, or with fewer than 3 usable neighbours, is flagged.
 *   - 3 <= k <= min(63, nt - 1) and 0 < angle_deg < 360, else OA_E_BAD_ARG.  The defaults of the bindings are 16 and 90.
 *
 * oa_target_boundary builds the masks if need be and copies them out; either pointer may be NULL.  k and angle_deg are ignored
 * for a mesh; edge_mask must be NULL for a cloud (OA_E_BAD_ARG).  OA_E_STATE without a target, and on a multi-device context
 * (single-device).  The masks are kept until a new target upload; a cloud's also until its normals or (k, angle_deg) change.
 * Ends a running oa_iterate sequence.
 *
 * oa_set_reject_boundary(on): a pair that pair_eval accepts (dist < thresh, and the normal-angle test when it is on) is dropped
 * when it lies on the boundary.  Surface mode: the closest point on the winning triangle lies on an edge whose bit is set, or on
 * a vertex whose mask is 1 (the region is oa_deviation's `feature`; a face is never on the boundary).  Vertex mode: the winning
 * vertex is flagged.  A step runs search -> [reciprocal check] -> boundary verdict -> [trim] -> [estimated robust scale] ->
 * accumulate; a rejected pair is rejected as the reciprocal check rejects one: it leaves the sums of all three metrics, the
 * weighted kernels, K, mean and std, the trim's candidates, the automatic scale's quantile, and oa_make_pairs.  oa_nn_search,
 * oa_deviation, oa_score_poses and the coarse stages do not look at the setting.  Fewer than 3 survivors is OA_E_TOO_FEW_PAIRS.
 * The masks are built before the loop starts, with the setting's (k, angle_deg): the setter checks 3 <= k <= 63 and the angle, the
 * build holds k against the target (k > nt - 1: OA_E_BAD_ARG from the loop, the context stays usable).  on == 0 (the default) changes nothing: the same
 * launches, the same bits.  The setting survives uploads and oa_set_matrices; changing it ends a running oa_iterate sequence.
 * Single-device contexts holding the whole selection: with the setting on, loops and oa_make_pairs of a multi-device context,
 * oa_run_begin / oa_iter_partial, and any loop over a source uploaded with shard_count > 1 fail with OA_E_STATE (the context
 * stays usable; oa_set_reject_boundary(ctx, 0, 16, 90) brings the plain pairs back). */
int oa_target_boundary(oa_ctx *ctx, int k, double angle_deg, uint8_t *vertex_mask, uint8_t *edge_mask);
int oa_set_reject_boundary(oa_ctx *ctx, int on, int k, double angle_deg);
/* EXTENSION: one weight per source vertex (host, float32, n_verts as uploaded with oa_set_source; finite and >= 0), gathered
 * into the selection's order -- "trust this region less", where vlist can only say yes or no.  w == NULL switches the weights
 * off (every w_vertex = 1); a new source upload forgets them.  OA_E_STATE before oa_set_source; OA_E_BAD_ARG for a count other
 * than the uploaded n_verts and for a negative or non-finite weight (the weights in force stay).  Multi-device contexts: every
 * child gathers its own shard. */
int oa_set_source_weights(oa_ctx *ctx, const float *w, int64_t n_verts);
/* matrix_world of the align and base objects (functions/general.py:262-263) */
int oa_set_matrices(oa_ctx *ctx, const float mx_align[16], const float mx_base[16]);
int oa_get_matrix_world(oa_ctx *ctx, float mx_align[16]);
/* Forget the correspondences of earlier searches (every search seeds itself with the previous answer of its slot: any
 * seed gives the same result, a good one gives it sooner).  A new upload does this by itself; oa_set_matrices does
 * not -- a host-driven make_pairs loop sets the matrices before every call and keeps its seeds.  Timing runs call it to
 * start cold. */
int oa_reset_seeds(oa_ctx *ctx);
/* Introspection (sizes of the search structures, for roofline arithmetic and tests). */
#define OA_STAT_GRID_CELLS        1   /* cells of the vertex grid (0 = none built) */
#define OA_STAT_TRI_GRID_CELLS    2   /* cells of the triangle grid */
#define OA_STAT_TRI_GRID_ENTRIES  3   /* (triangle, cell) entries of the triangle grid's cell lists */
#define OA_STAT_N_TRIS            4
#define OA_STAT_SURFACE           5   /* 1 = surface mode (oa_set_target_mesh) */
#define OA_STAT_CACHE_BYTES       6   /* device bytes currently held by the process-wide allocation cache */
#define OA_STAT_BRUTE_KERNEL      7   /* what OA_SEARCH_BRUTE launches for the current shard: 0 = k_nn_search (exact only), 1 =
                                       * k_nn_search_filtered (rounds 1-4; OA_NN_SORT=0), 2 = k_nn_search_mfma (experiment, env OA_NN_MFMA=1),
                                       * 3 = k_nn_search_sorted (default: the filtered search over the target sorted along its longest axis) */
#define OA_STAT_EXCHANGE          8   /* multi-device context: what its loops exchange through (resolves AUTO): 0 = mailbox in pinned
                                       * host memory, 1 = RCCL, 2 = mailboxes in peer-mapped device memory; -1 = not a multi context */
#define OA_STAT_RCCL_RANKS        9   /* ranks of the RCCL communicator the loops use (0 = RCCL not in use) */
#define OA_STAT_ENQUEUE_US       10   /* multi-device context: host time per iteration spent enqueuing ONE device's work in the
                                       * last oa_run (mean over iterations, max over devices), microseconds */
#define OA_STAT_HOST_THREADS     11   /* multi-device context: host threads that drive its devices (1 = the caller alone) */
#define OA_STAT_FAST_ITERATIONS  12   /* iterations of the last / current loop in which the grid search finished its own leftovers and
                                       * accumulated in its epilogue (the adaptive choice of docs/HISTORY.md 4.4; first device) */
#define OA_STAT_HANDOVER_ENTRIES 13   /* what the last grid search handed to the tree: queries ... */
#define OA_STAT_HANDOVER_WAVE_MAX 14  /* ... and the most any ONE wavefront handed over (what the adaptive choice looks at) */
#define OA_STAT_ENQUEUED_MIN      15   /* multi-device context: iterations the host enqueued for its children in the last oa_run, the */
#define OA_STAT_ENQUEUED_MAX      16   /* least and the most over the children.  Equal by construction (docs/HISTORY.md 4.7, "the invariant"):
                                       * in RCCL mode every enqueued iteration holds a collective every rank has to enter */
#define OA_STAT_WATCHDOG_ABORTS   17   /* times this context's RCCL communicators were aborted (watchdog / asynchronous error) */
#define OA_STAT_NN_MS_MIN         18   /* multi-device context: search time of the last oa_run (sum over its iterations, ms) on the */
#define OA_STAT_NN_MS_MAX         19   /* fastest / the slowest device: how evenly the shards load the GPUs */
#define OA_STAT_SAFE_RADII        20   /* 1 = the vertex grid's safe radii are built for the current target (a seed inside its own settles the
                                       * query without a scan or a descent, docs/HISTORY.md 4.4; built once the target has seen 8 loop iterations; first device) */
#define OA_STAT_TRI_RING          21   /* 1 = the triangle neighbour lists are built for the current mesh (a query within its seed triangle's accept
                                       * radius is settled by the seed and the triangles that touch it, docs/HISTORY.md 4.5; built once the mesh has
                                       * seen 4 loop searches, OA_TRI_RING=2: with the grid; first device) */
#define OA_STAT_TRI_RING_ACCEPTS  22   /* diagnostic (one extra launch + a wait): source points of this shard that the neighbour lists would settle at
                                       * the current pose with the current seeds; multi-device context: the sum over the shards */
#define OA_STAT_EXCHANGE_US       23   /* multi-GPU: mean time per iteration of the last loop a device spent between "its sums are ready" and "the
                                       * world's sums are in hand" (GPU-side stamps: the all-reduce, or the gather's wait), slowest device */
#define OA_STAT_RCCL_FALLBACKS    24   /* loops that AUTO began on RCCL and finished through the mailboxes (the watchdog aborted the communicators) */
#define OA_STAT_RCCL_RANKS_LAST   25   /* ranks of the last RCCL communicator that came up and passed its handshake -- still reported after a
                                       * fallback, when OA_STAT_RCCL_RANKS is back to 0 */
#define OA_STAT_SEARCH_CLOCK_MHZ   26   /* shader clock during the last loop's k_nn_search_sorted launch (cycle counter / constant-rate counter of one
                                       * workgroup dispatched mid-launch); 0 when that kernel did not run.  Multi-device context: its first device */
#define OA_STAT_BRUTE_QUEUE_WGS     27   /* workgroups of the last k_nn_search_sorted launch that took their (split, block) items off the work
                                       * queue (long launches: as many as the chip holds); 0 = one workgroup per item, in launch order */
#define OA_STAT_METRIC          28   /* OA_METRIC_POINT / OA_METRIC_PLANE / OA_METRIC_GICP / OA_METRIC_SYMMETRIC */
#define OA_STAT_PLANE_RANK      29   /* eigenvalues the last plane solve kept (6 = fully determined); loop, oa_point_to_plane or oa_symmetric_step */
#define OA_STAT_ROBUST_LOSS     30   /* OA_LOSS_* */
#define OA_STAT_WEIGHT_SUM      31   /* sum w of the last step (loop or iterate); K when weighting is off */
#define OA_STAT_ROBUST_SCALE    32   /* the c the last step used: oa_set_robust's scale, or c_i of oa_set_robust_auto; 0 with OA_LOSS_NONE */
#define OA_STAT_ROBUST_QUANTILE 33   /* oa_set_robust_auto's quantile (0 = off) */
#define OA_STAT_TARGET_NORMALS  34   /* 1 when a vertex-mode target has normals installed (oa_set_target_normals, oa_set_normals, an estimate) */
#define OA_STAT_TARGET_FEATURES 35   /* 1 when oa_target_fpfh(keep) left descriptors resident */
#define OA_STAT_MESH_PSEUDONORMALS 36 /* 1 when the mesh's pseudo-normals are built (oa_deviation, oa_get_mesh_pseudonormals); a new upload forgets them */
#define OA_STAT_RECIPROCAL      37   /* 1 when oa_set_reciprocal is on */
#define OA_STAT_RECIPROCAL_RATIO 38  /* its ratio */
#define OA_STAT_RECIP_REJECTED  39   /* pairs of the last step (loop, oa_iterate or oa_make_pairs) that passed everything else and failed the
                                      * reciprocal check; 0 when the check is off, and after oa_set_source or oa_set_reciprocal until a step runs */
#define OA_STAT_TRIM            40   /* oa_set_trim's setting: 0 (off), the fraction, or -1 (OA_TRIM_AUTO) */
#define OA_STAT_TRIM_CANDIDATES 41   /* K_q of the last step (loop, oa_iterate or oa_make_pairs); 0 when the trim is off, and after
                                      * oa_set_source or oa_set_trim until a step runs -- as are the next two */
#define OA_STAT_TRIM_KEPT       42   /* candidates of the last step that stayed */
#define OA_STAT_TRIM_CUT        43   /* the cut q of the last step, as a double; 0 when off or K_q = 0 */
#define OA_STAT_REJECT_BOUNDARY 44   /* 1 when oa_set_reject_boundary is on */
#define OA_STAT_BOUNDARY_REJECTED 45 /* pairs of the last step that passed everything before the verdict, the reciprocal check included,
                                      * and lay on the target's boundary; 0 when off, and after oa_set_source or oa_set_reject_boundary until a step runs */
#define OA_STAT_TARGET_BOUNDARY 46   /* 1 when the boundary masks are built for the current target */
#define OA_STAT_BOUNDARY_VERTICES 47 /* flagged vertices of the built masks (0 when not built) */
#define OA_STAT_BOUNDARY_EDGES  48   /* boundary edges of the built masks (0 for a cloud, or when not built) */
#define OA_STAT_ACC_PATH       49   /* which pair accumulation the last step (loop, oa_iterate, oa_iter_partial, oa_make_pairs) launched, OA_ACC_* below; 0 before
                                      * the first step.  A host integer written where the launch is decided: no device read.  First device */
#define OA_STAT_ACC_ROWS       50   /* rows of per-workgroup partials the last step's reduce launch was given (DUAL: the grid's rows; the tree's
                                      * are chosen on the device); 0 before the first step.  First device */
#define OA_STAT_TARGET_CLEANED 51   /* vertices the last oa_target_outliers(apply) or oa_target_clusters(apply) removed from the resident target; 0 after a plain upload */
#define OA_ACC_CANON            1  /* k_pair_accumulate_canon behind a search: one thread per (slot, lane of the query) */
#define OA_ACC_STRIDE           2   /* the grid-stride k_pair_accumulate */
#define OA_ACC_WEIGHTED         3   /* k_pair_accumulate_weighted */
#define OA_ACC_PLANE            4   /* k_pair_accumulate_plane; OA_METRIC_SYMMETRIC: its sibling k_pair_accumulate_symm (the same row and epilogue) */
#define OA_ACC_GICP             5   /* k_pair_accumulate_gicp */
#define OA_ACC_FUSED_GRID       6   /* the epilogue of the vertex grid search */
#define OA_ACC_FUSED_TRI_GRID   7   /* the epilogue of the triangle grid search */
#define OA_ACC_FUSED_TREE       8   /* the epilogue of the whole-shard tree search, vertex target */
#define OA_ACC_FUSED_TRI_TREE   9   /* ... mesh target */
#define OA_ACC_DUAL            10   /* tree and grid searches both enqueued, both accumulate; DevState::tree_turn picks on the device */
#define OA_STAT_ENQUEUED_CHILD  1000  /* + i: the same count for child i alone */
int oa_get_stat(oa_ctx *ctx, int what, double *value);
/* why the exchange is what it is (AUTO's reason for not taking RCCL, librccl's error, "RCCL was aborted: ..."), or "" */
const char *oa_exchange_note(oa_ctx *ctx);
int64_t oa_num_selected(oa_ctx *ctx);     /* selected source points held by this context (its shard) */

/* ---- contract 1: make_pairs (functions/general.py:257-329) ------------------------------------ */
/* A, B: caller-allocated 3 x cap row-major doubles (row = axis); pairs come out in vlist order.
 * dstats = [mean, population std] of the world-space pair distances when calc_stats. */
int oa_make_pairs(oa_ctx *ctx, double thresh, int calc_stats,
                  double *A, double *B, int64_t cap, int64_t *K, double dstats[2]);
/* the correspondence search alone: nearest target vertex index (surface mode: nearest triangle index) and fp32
 * squared distance (base-local) for every selected source point of this shard.  idx/d2 may be NULL (timing). */
int oa_nn_search(oa_ctx *ctx, int64_t *idx, float *d2, double *kernel_ms);

/* ---- contract 2: affine_matrix_from_points(v0=A, v1=B, shear=False, scale, usesvd=True)
 *      (functions/general.py:105-217); alias calc_target_matrix in the Python host ------------ */
/* A, B: 3 x K row-major doubles with leading dimension ld (host).  with_scale: bit 0 = uniform scale (scale=True); bit 1 = the
 * rotation through Horn's quaternion (usesvd=False, :191-206) instead of the SVD of the covariance (:179-190). */
int oa_kabsch(oa_ctx *ctx, const double *A, const double *B, int64_t K, int64_t ld,
              int with_scale, double M[16]);
/* The reference's full signature (functions/general.py:105): v0, v1 are ndims x K row-major doubles with leading
 * dimension ld (host), 2 <= ndims <= 64 (the reference takes any; 9 and more run through a device workspace); shear != 0: the affine (Hartley & Zisserman) branch (:168-178, the signature's
 * default), else rigid / similarity through the SVD of the covariance (:179-190, :208-212).  M: (ndims+1)^2 doubles,
 * row-major.  K < ndims or ndims < 2: OA_E_TOO_FEW_PAIRS, the reference's ValueError (:150-157). */
int oa_affine_from_points(oa_ctx *ctx, const double *v0, const double *v1, int ndims, int64_t K, int64_t ld,
                          int shear, int with_scale, double *M);
/* same solve from the OA_NSUMS accumulated sums (host array; layout: S_A .. S_DD in csrc/oa_kernels.hpp).  The sums are taken
 * relative to `pivot` (a' = a - pivot, b' = b - pivot); pivot == NULL means the origin. */
int oa_kabsch_from_sums(oa_ctx *ctx, const double sums[OA_NSUMS], const double pivot[3], int with_scale,
                        double M[16]);
/* the pivot this context subtracts before accumulating (the first selected source vertex) */
int oa_get_pivot(oa_ctx *ctx, double pivot[3]);

/* the plane step from caller-supplied pairs: A, B, N are 3 x K row-major doubles, leading dimension ld; N need not be unit.
 * Pivot c = A's first column (the loop's rule: first selected source vertex) -- the minimum-norm answer of a rank-deficient
 * system depends on the frame of (omega, t), so the pivot is part of the contract.  M maps A towards B's tangent planes
 * (the M of oa_kabsch's convention).  K < 3: OA_E_TOO_FEW_PAIRS.  Does not look at the context's metric. */
int oa_point_to_plane(oa_ctx *ctx, const double *A, const double *B, const double *N, int64_t K, int64_t ld, double M[16]);
/* the symmetric step (OA_METRIC_SYMMETRIC's) from caller-supplied pairs: A, B, NA, NB are 3 x K row-major doubles, leading
 * dimension ld; NA (the normals at A) and NB (at B) need not be unit -- they are normalised as the loop normalises its own, and
 * a pair with a normal of zero or non-finite length on either side is left out.  Pivot c = A's first column.  K < 3 (or fewer
 * than 3 usable pairs): OA_E_TOO_FEW_PAIRS.  Sets OA_STAT_PLANE_RANK.  Does not look at the context's metric. */
int oa_symmetric_step(oa_ctx *ctx, const double *A, const double *B, const double *NA, const double *NB, int64_t K, int64_t ld, double M[16]);

/* ---- fused fast path: the operator loop (operators/icp_align.py:91-151) ----------------------- */
/* one iteration, synchronous (the modal operator's per-tick step, icp_align_feedback.py:250-288):
 * M_step = this iteration's 4x4 (float64); stats = [K, mean_dist, std_dist, |translation|, rot_angle, converged].
 * A sequence of calls with the same thresh / target_d / use_target / with_scale is one loop (n counts up, the 5-slot
 * convergence ring fills).  Different settings, or any call in between that re-stages the device state
 * (oa_set_matrices, oa_make_pairs, oa_nn_search, oa_run, a new upload), start a new sequence -- n = 0, fresh ring --
 * from the current matrix_world.  History: the last 64 iterations of the sequence. */
int oa_iterate(oa_ctx *ctx, const oa_settings *st, double M_step[16], double stats[6]);
/* the whole loop, device resident (no host round trip per iteration) */
int oa_run(oa_ctx *ctx, const oa_settings *st, oa_report *rep);
/* per-iteration history of the last oa_run (its first max_n iterations) / oa_iterate sequence (its last max_n,
 * oldest first) -- each array may be NULL:
 * step_M n x 16 doubles, step_new n x 16 floats (new_mat, operators/icp_align.py:116-119),
 * step_K n, step_stats n x 2, step_trans n.  Returns the number of iterations recorded. */
int oa_get_history(oa_ctx *ctx, int32_t max_n, double *step_M, float *step_new,
                   int64_t *step_K, double *step_stats, double *step_trans);

/* search time (ms) of every iteration of the last oa_run / oa_run_end -- what oa_report::nn_ms_total sums; returns how many
 * were written (<= max_n).  Multi-device context: its first device.  (bench.py: per-launch min / median / max) */
int oa_get_search_ms(oa_ctx *ctx, int32_t max_n, double *ms);
/* Diagnostic for bench.py's roofline (no counterpart in the reference): what the vector ALUs issue right now -- ~target_ms of
 * independent v_add_f32 / v_min3_f32 chains on every SIMD, 8 waves each.  out[0] = T lane-ops/s of v_add_f32 (two register
 * sources: the issue rate itself), out[1] = shader clock in MHz during that burn, out[2] = duration in ms, out[3] = T lane-ops/s
 * of v_min3_f32 (the half-rate class: v_min_f32, v_min3_f32, v_cmp_*_f32).  The brute-force search is bound by exactly these
 * rates, weighted by its instruction mix. */
int oa_measure_valu_ceiling(oa_ctx *ctx, double target_ms, double out[4]);

/* ---- split-phase loop for one-process-per-GPU sharding ---------------------------------------- */
/* oa_run_begin resets the loop state (ring buffer, counters) on the device. */
int oa_run_begin(oa_ctx *ctx, const oa_settings *st);
/* enqueue correspondence search + pair accumulation for this shard; the OA_NSUMS partial sums
 * land in d_sums (DEVICE pointer, e.g. a torch tensor) ready for an all-reduce(sum). */
int oa_iter_partial(oa_ctx *ctx, double *d_sums);
/* enqueue solve + matrix_world update + convergence ring from the (all-reduced) sums. */
int oa_iter_finish(oa_ctx *ctx, const double *d_sums);
/* synchronise and fetch the report. */
int oa_run_end(oa_ctx *ctx, oa_report *rep);

/* ---- EXTENSION: coarse global alignment (no counterpart in the reference, whose only remedy for a bad start is picking
 *      landmarks by hand, operators/align_pick_points.py) -- DESIGN.md 3.11 ------------------------------------------ */
/* Scores of n_poses candidate align matrices (host, n_poses x 16 float32, row-major) in ONE launch: per pose a cold nearest-
 * primitive query (vertex or surface mode, the context's correspondence rule, through the target's box tree) for every sample
 * point -- the selection's points whose position in the caller's (vlist) order is a multiple of stride (stride <= 1: all; S of
 * them) -- with the pose in place of matrix_world: the query is co_find's, the distance and its test `dist < thresh` are
 * make_pairs'.  No normal-angle test, no weights.  Per pose, OA_POSE_NSCORE doubles:
 *   K          sample points with dist < thresh
 *   mean_dist  } the d_stats oa_make_pairs(thresh, calc_stats = 1) reports for that pose and that sample (population std);
 *   std_dist   } NaN when K = 0
 *   cost       (sum of the passing dist + (S - K) thresh) / S: the mean of min(dist, thresh); finite, lower is better
 * Fixed-order fp64 sums: the same bits on every run.  No side effects: the call reads the base matrix of oa_set_matrices and
 * writes nothing a loop reads -- a running oa_iterate sequence continues, a later oa_run returns the bits it would have.
 * OA_E_STATE without target, source or matrices, without the box tree (OA_SEARCH_BRUTE), with an empty selection, and on a
 * multi-device context; OA_E_BAD_THRESH for thresh <= 0; OA_E_BAD_ARG for null pointers, n_poses outside 1 .. 65536, a non-finite
 * entry, or S x n_poses >= 2^31. */
#define OA_POSE_NSCORE 4   /* per pose: K, mean_dist, std_dist, cost */
int oa_score_poses(oa_ctx *ctx, const float *mx_align /* n_poses x 16, host */, int32_t n_poses,
                   double thresh, int32_t stride, double *scores /* n_poses x OA_POSE_NSCORE */);
/* n_rot candidate align matrices: candidate k = float32(T(c_t) R_k T(-c_s) mx_align), formed in fp64; c_s = the world-space
 * centroid of the selected source points under the current matrix_world (oa_get_matrix_world), c_t = that of the target's
 * vertices (sums of the float32 matrix @ vertex products, accumulated in fp64 on the device in a fixed order); R_k = rotation k
 * of the n_rot-point super-Fibonacci set on SO(3) (Alexa 2022): s = k + 1/2, r = sqrt(s/n), R = sqrt(1 - s/n),
 * alpha = 2 pi s / sqrt(2), beta = 2 pi s / 1.533751168755204288118041, quaternion (x, y, z, w) = (r sin alpha, r cos alpha,
 * R sin beta, R cos beta).  1 <= n_rot <= 65536.  No side effects; single-device contexts. */
int oa_coarse_candidates(oa_ctx *ctx, int32_t n_rot, float *mx_align_out /* n_rot x 16 */);
typedef struct oa_coarse_settings {
    int32_t n_rot;         /* rotation candidates (256) */
    int32_t n_refine;      /* best candidates that get a short loop (8) */
    int32_t refine_iters;  /* iterations of that loop (10) */
    int32_t stride;        /* sample stride for scoring and refining (4) */
    double  thresh;        /* truncation / pair distance of the coarse stage, world units */
} oa_coarse_settings;
typedef struct oa_coarse_report {
    int32_t n_candidates, best_candidate, best_rank, status;   /* best_candidate: the winner's origin (n_candidates = the incoming pose); best_rank: its place among the first scores */
    double  cost_start, cost_best_candidate, cost_refined;     /* cost of the incoming pose, of the winner before and after its loop */
    int64_t K_refined;
    double  score_ms, total_ms;                                /* host time of the first scoring call / of the whole call */
} oa_coarse_report;
/* Multi-start: oa_coarse_candidates(n_rot) plus the incoming pose -> one scoring launch -> the n_refine lowest costs (ties to
 * the lower index; the incoming pose always among them) each get refine_iters iterations of the plain point loop over the
 * sample (thresh, rigid, no early exit; never the context's metric, loss, weights or normal test; a step with fewer than three
 * pairs leaves its pose where it is) -> one more scoring launch -> matrix_world becomes the lowest cost, so that the caller's
 * oa_run starts there.  When nothing beats the incoming pose it stays in force.  The refinement runs on kernels of its own, all
 * poses at once: the selection, the seeds (kept, not reset), the metric and the robust settings are not touched.  Ends a
 * running oa_iterate sequence, as oa_set_matrices does.  Single-device contexts (else OA_E_STATE); OA_E_BAD_THRESH for
 * thresh <= 0, OA_E_BAD_ARG for n_rot outside 1 .. 65536, n_refine outside 1 .. 4096, refine_iters outside 0 .. 10000. */
int oa_coarse_align(oa_ctx *ctx, const oa_coarse_settings *cs, oa_coarse_report *rep);
/* The recipe of oa_coarse_align with the candidates supplied instead of generated: mx_align (n_poses x 16 float32, host; 1 ..
 * 65535 of them, every entry finite) plus the incoming pose -> one scoring launch -> the n_refine best -> refine_iters x (score,
 * solve) -> rescore -> matrix_world = the lowest cost, or the incoming pose when nothing beats it.  cs->n_rot is ignored;
 * rep->n_candidates = n_poses, and best_candidate = n_poses names the incoming pose.  Fed oa_coarse_candidates(n)'s output it
 * leaves the bits oa_coarse_align(n_rot = n) leaves.  Everything else as oa_coarse_align. */
int oa_coarse_align_poses(oa_ctx *ctx, const float *mx_align /* n_poses x 16, host */, int32_t n_poses,
                          const oa_coarse_settings *cs, oa_coarse_report *rep);

/* ---- EXTENSION: candidate poses from matched descriptors, for sources that are a PART of the target (their centroids are far
 *      apart: no rotation about the centroid is near the answer) -- DESIGN.md 3.14.  The matching takes any local shape
 *      descriptor of up to 64 floats per vertex; the library's own is FPFH (33). ------------------------------------------------- */
/* Fast Point Feature Histograms (Rusu, Blodow & Beetz 2009) of the resident vertex-mode target: out (nt x 33 float32, host, may
 * be NULL), from every vertex's k nearest neighbours in the order of oa_target_knn (4 <= k <= min(64, nt)) and the target's
 * normals (oa_set_target_normals, oa_set_normals or an installed estimate; OA_E_STATE without them, on a surface target and on
 * a multi-device context).  fp64 arithmetic, sums in list order, one rounding to float32:
 *   pair feature of vertex p (normal n_p) and list neighbour q != p (normal n_q): d = q - p, l = |d|; skipped when l = 0 or not
 *     finite or when a normal is zero (or not finite).  e = d / l.  If |n_p.e| < |n_q.e|: (n1, n2, e) = (n_q, n_p, -e), else
 *     (n_p, n_q, e).  f3 = n1.e, v = e x n1 (the pair is skipped when |v| = 0), v <- v / |v|, w = n1 x v, f2 = v.n2,
 *     f1 = atan2(w.n2, n1.n2).  Bins floor(11 (f1 + pi) / 2 pi), floor(11 (f2 + 1) / 2), floor(11 (f3 + 1) / 2), clamped to 0 .. 10.
 *   SPFH(p), 3 x 11 bins: (pairs in the bin) x (100 / m), m = p's number of valid pairs; m = 0: the zero row.
 *   FPFH(p) = SPFH(p) + (1 / m) sum over p's valid pairs of SPFH(q) / l_q^2; then every third is scaled to sum to 100 (a third
 *     that sums to 0 stays zero).  A vertex with a zero normal, a non-finite coordinate or m = 0 has the zero row: "no descriptor".
 * No atomics: the same bits on every call.  keep != 0 leaves the descriptors resident for oa_feature_candidates(tgt_feat =
 * NULL); a new target forgets them.  Ends a running sequence, as oa_estimate_target_normals does. */
int oa_target_fpfh(oa_ctx *ctx, int k, float *out /* nt x 33, or NULL */, int keep);
/* For every row of fa (na x dim float32, host) the row of fb (nb x dim) at the smallest squared L2 distance, that distance
 * and the second smallest distance (it feeds a ratio test; with exact duplicates in fb it equals the smallest).  The distance
 * is the float32 sum, in column order, of the squared float32 differences; ties go to the lowest index.  Rows that are entirely
 * zero mean "no descriptor": they neither query nor answer -- index -1, both distances +inf; so does a query with no row left
 * to answer, and the second distance is +inf when only one row answers.  The same bits on every run.  Outputs may be NULL.
 * Needs no target, source or matrices.  OA_E_BAD_ARG: dim outside 1 .. 64, na or nb outside 1 .. 2^24; OA_E_STATE on a
 * multi-device context. */
int oa_match_features(oa_ctx *ctx, const float *fa, int64_t na, const float *fb, int64_t nb, int32_t dim,
                      int32_t *out_idx /* na */, float *out_d2 /* na */, float *out_d2_second /* na */);
typedef struct oa_feature_settings {
    int32_t  dim;        /* floats per descriptor row, 1 .. 64 (33) */
    int32_t  n_hyp;      /* hypotheses = triples of kept pairs, 1 .. 65535 (4096) */
    int32_t  mutual;     /* 1: a pair must be the nearest row in both directions AND pass the ratio test; 0: the ratio test alone (1) */
    uint32_t seed;       /* of the hashed draw (0) */
    double   ratio;      /* keep (s, t) when d2 <= ratio^2 d2_second; a ratio >= 1 switches the test off (0.9) */
    double   edge_tol;   /* a triple's three edge-length ratios |a_i - a_j| / |b_i - b_j| must lie in [edge_tol, 1 / edge_tol] (0.9) */
    double   min_edge;   /* shortest edge on either side, world units; <= 0: 0.05 x the diagonal of the target's bounding box */
} oa_feature_settings;
#define OA_FEAT_TOO_FEW_PAIRS 1   /* oa_feature_report::status: fewer than three pairs were kept */
#define OA_FEAT_NO_POSE       2   /* every hypothesis was rejected */
typedef struct oa_feature_report {
    int32_t n_pairs, n_accepted, status, reserved;   /* pairs kept; hypotheses that gave a pose (= *n_out); OA_OK or OA_FEAT_* */
    double  match_ms, total_ms;                      /* host time of the matching / of the whole call */
} oa_feature_report;
/* src_feat: n_verts x dim in the caller's source vertex order, as oa_set_source_normals takes its rows; only the selection's
 * rows are used.  tgt_feat: nt x dim in the target's vertex order; NULL: the descriptors oa_target_fpfh kept (dim must be
 * 33; OA_E_STATE when there are none).  Vertex-mode targets, single-device contexts (else OA_E_STATE).
 *  1. oa_match_features selection -> target (and target -> selection when `mutual`); the kept pairs (see the settings) are
 *     ordered by source vertex index.  Fewer than three: *n_out = 0, status OA_FEAT_TOO_FEW_PAIRS, the call returns OA_OK.
 *  2. World-space points a = matrix_world @ src, b = mx_base @ tgt (the float32 products of the loop).
 *  3. n_hyp triples of pair indices: `triples` (n_hyp x 3 int32; an index outside 0 .. n_pairs - 1 rejects the hypothesis), or,
 *     when NULL, index = hash(seed, hypothesis h, position k = 0, 1, 2) in uint32 arithmetic (wrapping):
 *       x = seed ^ (h * 0x9E3779B9) ^ ((k + 1) * 0x85EBCA6B)
 *       x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
 *       index = (uint64(x) * n_pairs) >> 32
 *  4. A hypothesis is rejected when two of its indices coincide, when an edge on either side is shorter than min_edge, when an
 *     edge ratio leaves [edge_tol, 1 / edge_tol], or when the solve fails.  Else M = the rigid least-squares motion a -> b of its
 *     three pairs (the loop's solve on sums taken about a_0) and the candidate is float32(M @ mx_align), formed in fp64.
 *  5. mx_align_out (room for n_hyp x 16) receives the accepted candidates in hypothesis order, *n_out their number.
 * No side effects, as oa_coarse_candidates. */
int oa_feature_candidates(oa_ctx *ctx, const float *src_feat, int64_t n_verts, const float *tgt_feat,
                          const oa_feature_settings *settings, const int32_t *triples /* n_hyp x 3, or NULL */,
                          float *mx_align_out /* n_hyp x 16 */, int32_t *n_out, oa_feature_report *report);

/* ---- EXTENSION: voxel-grid downsampling -- spatially uniform thinning of a cloud, where oa_set_source's stride thins by index
 *      and keeps the density skew of a scan -- DESIGN.md 3.15.  Needs no target, source or matrices (as oa_match_features) and
 *      touches nothing a loop reads: a running oa_iterate sequence continues with the bits it would have had.  OA_E_STATE on a
 *      multi-device context. ------------------------------------------------------------------------------------------------- */
typedef struct oa_voxel_report {
    int64_t n_in, n_finite, n_voxels;   /* points given; with three finite coordinates; occupied voxels */
    int64_t max_members;                /* most points in one voxel */
    int32_t dims[3]; int32_t reserved;  /* cells per axis */
    double  origin[3];                  /* the origin used */
    double  total_ms;                   /* host time of the call */
} oa_voxel_report;
/* xyz: n x 3 float32, host or (on_device != 0) device memory; normals: n x 3 on the same side, or NULL.  Outputs: host memory,
 * each may be NULL.
 * Cells.  A point with a non-finite coordinate takes no part (it is counted in n_in - n_finite).  Origin o: the caller's, or
 * (NULL) the componentwise minimum of the finite points.  Per axis, in fp64: c = floor(((double)x - o) / voxel) -- an IEEE
 * subtraction, an IEEE division and floor.  dims[a] = max c_a + 1; key = (c_z dims_y + c_y) dims_x + c_x, a 64-bit integer.
 * OA_E_BAD_ARG: voxel not finite and > 0; n outside 1 .. 2^31 - 2^20; normals without out_normals; a non-finite origin; with a
 * caller's origin, a point with a negative c; a dims[a] above 2^21; no finite point.
 * Rows: one per occupied voxel, in ascending key order; members = the voxel's points.
 *   out_xyz      the members' mean: per coordinate an fp64 sum, divided once by the count in fp64, rounded once to float32
 *   out_count    the number of members
 *   out_rep      the original index of the member nearest to the row's FLOAT32 mean: d2 = (dx dx + dy dy) + dz dz in fp64 with
 *                dx = (double)x - (double)mean32_x, no fused multiply-add; ties go to the lowest index
 *   out_normals  (when normals are given) the fp64 sum of the members' normals, normalised in fp64 as n * (1 / sqrt((x x + y y) +
 *                z z)) and rounded once; a sum of zero or non-finite length gives (0, 0, 0)
 * The order of the sums depends on the input alone -- no float atomics, two calls give the same bits -- and is, for a row of L
 * members listed by ascending original index m_0 < m_1 < ...:
 *   L <= 512: eight sums s_j = m_j + m_(j+8) + m_(j+16) + ... (each from +0, ascending), joined as
 *             ((s_0 + s_4) + (s_2 + s_6)) + ((s_1 + s_5) + (s_3 + s_7));
 *   L >  512: the list is cut into chunks of 512 (the last one shorter); per chunk 64 sums s_l = m_l + m_(l+64) + ..., joined by
 *             the butterfly t_l = s_l + s_(l ^ 32), then strides 16, 8, 4, 2, 1 likewise; the chunks' sums are added in chunk
 *             order, from +0.
 * Whenever the members' fp64 sum is exact (float32 values within one voxel share their exponent range: nearly always), the
 * result is that of any order.
 * *n_out = n_voxels (<= n_finite).  cap < n_voxels: OA_E_CAPACITY with *n_out and the report filled and no rows written.  Only
 * n_voxels rows are copied to the host. */
int oa_voxel_downsample(oa_ctx *ctx, const float *xyz, int64_t n, int on_device, const float *normals /* n x 3 or NULL, same side as xyz */,
                        double voxel, const double origin[3] /* or NULL */, int64_t cap,
                        float *out_xyz /* cap x 3 */, float *out_normals /* cap x 3 */, int32_t *out_count /* cap */,
                        int64_t *out_rep /* cap */, int64_t *n_out, oa_voxel_report *rep);

/* ---- EXTENSION: the deviation report -- how good is this alignment, and where does it deviate?    The loop's
 *      report carries the mean of the last step's pairs UNDER thresh, so a pose that lost half of its overlap reports a better
 *      mean; this call measures every selected point at the pose in force and says on which side of the target it lies. ----------- */
typedef struct oa_deviation_settings {
    double  thresh;         /* inlier test dist < thresh (the reference's); +inf: every pair is an inlier.  Must be > 0 */
    int32_t signed_mode;    /* -1 signed when possible (default), 0 never, 1 required (OA_E_STATE for a vertex-mode target without normals) */
    int32_t n_quantiles;    /* 0 .. 8 */
    double  quantiles[8];   /* each in (0, 1] */
    int32_t n_bins;         /* 0 .. 1024 histogram bins over [hist_lo, hist_hi) of signed_d; 0 = no histogram */
    int32_t reserved;
    double  hist_lo, hist_hi;
} oa_deviation_settings;
typedef struct oa_deviation_report {
    int64_t n, n_valid, n_inlier;   /* slots; with a correspondence; with dist < thresh */
    int64_t n_inside, n_unsigned;   /* signed_d < 0; signed slots whose normal was zero or not finite (they count as +dist) */
    int64_t max_index;              /* lowest caller-order position that attains max_dist (-1: no valid slot) */
    double  fitness;                /* n_inlier / n */
    double  mean, rms, std, mean_signed;   /* over the inliers; std = sqrt(max(rms^2 - mean^2, 0)); NaN without inliers */
    double  max_dist;               /* over the valid slots: the one-sided Hausdorff distance source -> target */
    double  quantile_values[8];     /* value k: the ceil(q_k n_valid)-th smallest of (float)dist over the valid slots */
    int32_t n_quantiles;
    int32_t signed_used;            /* 0 unsigned, 1 the mesh's pseudo-normals, 2 the target vertices' normals */
    int32_t surface, reserved;      /* 1: surface mode */
    double  search_ms, total_ms;    /* device time of the search; host time of the call */
    double  pseudonormal_ms;        /* host time of the pseudo-normal build when this call did it, else 0 */
} oa_deviation_report;
/* At the context's current matrix_world / mx_base, over the selected source points of the shard: ONE correspondence search (any
 * search mode, seeded or cold: the same answer), then for every slot, in the caller's (vlist) order -- every output pointer may
 * be NULL:
 *   idx       int64      what oa_nn_search returns for the slot; -1 = no correspondence (a non-finite source point)
 *   closest   float32 x3 co1: the closest point on triangle idx (surface mode; closest_on_tri's bits) or target vertex idx, base-local
 *   dist      float64    the world-space pair distance exactly as the accumulation kernels form it (the same bits); NaN without a
 *                        correspondence (closest and signed_d are NaN there too)
 *   signed_d  float64    dist with the sign below
 *   feature   int8       surface mode: where on the triangle the closest point lies -- 0 face; 1 / 2 / 3 edge ab / bc / ca; 4 / 5 / 6
 *                        vertex a / b / c (the region closest_on_tri's tests end in).  Vertex mode or no correspondence: -1
 * Sign.  p = co_find, r = co1 (float32, base-local), N the angle-weighted pseudo-normal (Baerentzen & Aanaes 2005) of the feature:
 *   s = ((p - r)_x N_x + (p - r)_y N_y) + (p - r)_z N_z in fp64;  signed_d = -dist if s < 0, else +dist.
 * Outside a counter-clockwise-wound (Blender's convention) closed mesh is positive.  A zero or non-finite N gives +dist and the
 * slot is counted in n_unsigned.  The sign is decided in base-local space: a mirrored mx_base does not flip it.
 * Pseudo-normals of the mesh: built on the device once per mesh, at the first signed call; a new upload forgets them
 * (OA_STAT_MESH_PSEUDONORMALS).  fp64 arithmetic on the float32 vertices, no fused multiply-add, no atomics -- two builds give the
 * same bits:
 *   n_t  = cross(b - a, c - a) * (1 / sqrt((x x + y y) + z z)); a triangle whose squared length is zero or not finite has
 *          n_t = 0 and corner angles 0: it takes part in nothing
 *   corner angle = atan2(|u x v|, u . v), u and v the corner's two edges
 *   N_v  = sum angle n_t over the corners at vertex INDEX v, added in ascending (triangle, corner) order
 *   N_uv = sum n_t over ALL triangles that have the undirected edge {u, v} (matched by vertex index), in ascending triangle order:
 *          the same bits for every triangle of the edge; a boundary edge has its one face, a non-manifold edge all of them
 * Faces use n_t in fp64; N_v and N_uv are stored as float32 (what oa_get_mesh_pseudonormals returns) and widened.
 * Vertex mode: N = the target vertex's normal (oa_set_target_normals, oa_set_normals, an estimate); without normals the result is
 * unsigned (signed_d = dist, signed_used = 0) -- or, with signed_mode = 1, OA_E_STATE.
 * Statistics (oa_deviation_report): integer counts, fixed-order fp64 sums (the same bits on every run and in every search mode);
 * the quantiles are exact order statistics by the rule and the radix select of oa_set_robust_auto.  Histogram (hist: n_bins + 2
 * int64 counts, the first for signed_d < hist_lo, the last for signed_d >= hist_hi): a valid slot with lo <= d < hi goes to bin
 * min(floor((d - lo) * (n_bins / (hi - lo))), n_bins - 1), fp64.
 * The call does not look at the normal-angle test, the robust loss, the weights or the metric.  It stages the device state as
 * oa_nn_search does (a running oa_iterate sequence ends).  OA_E_STATE on a multi-device context (it stays usable);
 * OA_E_BAD_THRESH for a thresh that is not > 0; OA_E_BAD_ARG for the other settings out of range. */
int oa_deviation(oa_ctx *ctx, const oa_deviation_settings *settings, double *signed_d, double *dist, float *closest /* n x 3 */,
                 int64_t *idx, int8_t *feature, int64_t *hist /* n_bins + 2 */, oa_deviation_report *report);
/* the mesh's pseudo-normals (built if needed): vertex_n nt x 3, edge_n n_tris x 3 edges (ab, bc, ca) x 3, host, either may be
 * NULL.  OA_E_STATE without a mesh target. */
int oa_get_mesh_pseudonormals(oa_ctx *ctx, float *vertex_n /* nv x 3 */, float *edge_n /* nt x 3 x 3 */);

/* ---- EXTENSION: normal-space sampling and the stability report of a selection -- which points enter the loop, and which motions
 *      they leave free.  Both calls need no target, source or matrices and touch nothing a loop reads (as
 *      oa_voxel_downsample); OA_E_STATE on a multi-device context.  Inputs: host arrays or (on_device != 0) device memory;
 *      outputs: host memory. ------------------------------------------------------------------------------------------------ */
typedef struct oa_sample_report {
    int64_t n_in, n_eligible;       /* normals given; those that take part */
    int64_t bins_occupied;          /* bins with at least one member */
    int64_t level;                  /* t below; the largest count when every eligible point is given */
    int64_t max_bin_count;          /* most members of one bin */
    double  total_ms;               /* host time of the call */
} oa_sample_report;
/* Normal-space sampling (Rusinkiewicz & Levoy 2001, 3.1): bucket the normals, draw evenly across the buckets -- m points of n,
 * as ascending original indices (a vlist for oa_set_source).  Every formula is plain IEEE fp64 with the grouping written, no fused
 * multiply-add; no float is ever added to another, and two calls give the same bits.
 * Eligible: a normal with three finite components whose l2 = (x x + y y) + z z, in fp64, is finite and > 0.
 * Bin (G = grid): a = the axis of the largest |component| (ties: the lowest axis), b = (a + 1) % 3, c = (a + 2) % 3.
 *   unoriented == 0: face f = 2 a + (n_a < 0), u = n_b / |n_a|, v = n_c / |n_a|   (6 G G bins)
 *   unoriented != 0: face f = a, u = n_b / n_a, v = n_c / n_a                     (3 G G bins; n and -n share a bin)
 *   iu = min(G - 1, (int)floor((u + 1.0) * (0.5 * G))), iv likewise from v; bin = (f G + iv) G + iu.
 * No square root and no normalisation: the bin depends on the direction alone.
 * Order inside a bin: ascending h(i) = (uint32)((i ^ seed) * 0x9E3779B1u), a bijection of the index: no ties.
 * Shares: with the bins' counts c_b, the level t is the largest integer with sum_b min(c_b, t) <= m; the remainder
 * r = m - sum_b min(c_b, t) goes one each to the first r bins, in ascending bin id, with c_b > t.  Bin b gives its first
 * min(c_b, t) (+ 1) members in hash order.  m >= n_eligible: every eligible point is given and level = max_bin_count.
 * out_idx (room for cap): the points given, ascending; *n_out = min(m, n_eligible) their number.  out_bin: n entries or NULL, the
 * bin of every point, -1 for one that is not eligible.
 * OA_E_BAD_ARG: m < 1; grid outside 1 .. 32; n outside 1 .. 2^31 - 2^20; no eligible point.  cap < *n_out: OA_E_CAPACITY with
 * *n_out and the report filled and nothing written to out_idx or out_bin. */
int oa_normal_space_sample(oa_ctx *ctx, const float *normals /* n x 3 */, int64_t n, int on_device, int64_t m, int32_t grid,
                           int32_t unoriented, uint32_t seed, int64_t cap, int64_t *out_idx /* cap */, int32_t *out_bin /* n, or NULL */,
                           int64_t *n_out, oa_sample_report *rep);

typedef struct oa_stability_report {
    int64_t n_used;                 /* eligible points among those analysed */
    double  centroid[3];            /* c */
    double  scale;                  /* s; 0 when the mean distance to c is 0 or not finite */
    double  C[36];                  /* row-major, symmetric */
    double  eigenvalues[6];         /* descending */
    double  eigenvectors[36];       /* row-major; COLUMN k belongs to eigenvalues[k] */
    int32_t rank, reserved;         /* eigenvalues > 1e-10 x the largest; 0 when scale is 0 */
    double  cond;                   /* eigenvalues[0] / eigenvalues[5]; +inf when eigenvalues[5] <= 0 or scale is 0 */
    double  total_ms;               /* host time of the call */
} oa_stability_report;
/* The 6 x 6 constraint matrix of a selection under the point-to-plane metric (Gelfand, Ikemoto, Rusinkiewicz & Levoy 2003) and
 * its eigen-decomposition: which rigid motions the selection resists.  xyz, normals: n x 3 float32 on the same side; idx: NULL
 * (all n points) or n_idx HOST indices in 0 .. n - 1 (a point listed twice counts twice).
 * Eligible: the normal as for oa_normal_space_sample, and three finite coordinates.  Over the eligible points, all fp64:
 *   c = (sum p) / n_used per coordinate;  s = 1 / ((sum sqrt((dx dx + dy dy) + dz dz)) / n_used), d = (double)p - c
 *   nh = n * (1 / sqrt(l2));  q = ((double)p - c) * s
 *   v = [q x nh ; nh], the cross product (q_y nh_z - q_z nh_y, q_z nh_x - q_x nh_z, q_x nh_y - q_y nh_x);  C = sum v v^T.
 * The order of the sums depends on the input alone -- no atomics, two calls give the same bits.  With N the number of points
 * analysed (n_idx, or n), B = min(256, ceil(N / 256)) and the points taken in the order given: sum g of 256 B adds the points at
 * positions g, g + 256 B, g + 512 B, ... in ascending order, from +0 (a point that is not eligible adds nothing); the sums
 * 64 k .. 64 k + 63 are joined by the butterfly t_l = s_l + s_(l ^ 32), then strides 16, 8, 4, 2, 1 likewise, into w_k; block b
 * of four gives ((w_4b + w_4b+1) + w_4b+2) + w_4b+3; then 64 sums z_l = block l + block (l + 64) + ... joined by the same butterfly.
 * Eigenvalues by cyclic Jacobi rotations in fp64, descending; eigenvector k is column k, signed so that its component of largest
 * magnitude (the lowest index on ties) is positive.  Rows 0-2 of a vector: a rotation about c in the normalised units (lengths
 * times s); rows 3-5: a translation.  A small eigenvalue: the selection does not resist that screw motion.
 * OA_E_BAD_ARG: n or n_idx outside 1 .. 2^31 - 2^20; an index outside 0 .. n - 1; no eligible point. */
int oa_stability(oa_ctx *ctx, const float *xyz, const float *normals, int64_t n, int on_device, const int64_t *idx /* host, or NULL */,
                 int64_t n_idx, oa_stability_report *rep);

#ifdef __cplusplus
}
#endif
#endif /* OA_ICP_H */
