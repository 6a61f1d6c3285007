"""IcpEngine: thin Python object over one `oa_ctx` (one GPU).

Holds no arithmetic of its own -- every number comes back from liboa_icp.so.
"""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager
from dataclasses import dataclass

import numpy as np

from . import _capi as capi

REF_VALUEERROR = "input arrays are of wrong shape or type"    # functions/general.py:157


@dataclass
class RunResult:
    iters_done: int
    converged: bool
    matrix_world: np.ndarray          # float32 4x4: align_obj.matrix_world after the loop
    last_K: int
    last_translation: float
    mean_dist: float
    std_dist: float
    mean_rot_angle: float
    nn_ms_total: float
    loop_ms: float
    step_M: np.ndarray                # n x 4 x 4 float64, the per-iteration affine_matrix_from_points result
    step_new: np.ndarray              # n x 4 x 4 float32, new_mat (operators/icp_align.py:116-119)
    step_K: np.ndarray
    step_stats: np.ndarray            # n x 2 [mean, std]
    step_trans: np.ndarray
    deviation: dict | None = None     # IcpAlign.run(..., deviation=DeviationSettings()): IcpEngine.deviation at the final pose


def _device_ptr(x):
    """(pointer, on_device, keepalive) for a numpy array or a torch tensor."""
    if hasattr(x, "data_ptr") and hasattr(x, "is_cuda"):          # torch tensor, without importing torch
        if x.is_cuda:
            import torch
            t = x.detach().to(dtype=torch.float32).contiguous().reshape(-1, 3)
            # the library reads the tensor on its own stream: whatever produced it on torch's stream (including the
            # conversion above) has to be finished first
            torch.cuda.current_stream(t.device).synchronize()
            return C.c_void_p(t.data_ptr()), 1, t, t.shape[0]
        x = x.detach().cpu().numpy()
    a = capi.as_f32(np.asarray(x)).reshape(-1, 3)
    return C.c_void_p(a.ctypes.data), 0, a, a.shape[0]


def _fpfh_k(k):
    if int(k) != k or not 4 <= int(k) <= 64:
        raise ValueError("fpfh: k = %r outside 4 .. 64" % (k,))
    return int(k)


def _feature_rows(f, name):
    """(n, dim) float32 descriptor rows, checked before any call reaches the library."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    if f.ndim != 2 or f.shape[0] < 1 or not 1 <= f.shape[1] <= 64:
        raise ValueError("%s: descriptor rows must be (n >= 1, 1 <= dim <= 64), got shape %s" % (name, f.shape))
    return f


def _voxel_args(xyz, voxel, normals, origin, name="voxel_downsample"):
    """The arguments of a voxel downsample, checked before any call reaches the library: (xyz, normals, origin) with host
    arrays made contiguous float32 (n, 3) and torch device tensors left as they are."""
    if isinstance(voxel, bool) or not isinstance(voxel, (int, float, np.integer, np.floating)) or not (np.isfinite(voxel) and voxel > 0):
        raise ValueError("%s: voxel = %r (finite and > 0)" % (name, voxel))

    def points(a, what):
        if hasattr(a, "data_ptr") and hasattr(a, "is_cuda"):      # torch tensor, without importing torch
            if a.dim() != 2 or a.shape[1] != 3 or a.shape[0] < 1 or "float32" not in str(a.dtype):
                raise ValueError("%s: %s must be (n >= 1, 3) float32, got %s %s" % (name, what, tuple(a.shape), a.dtype))
            return a
        a = np.asarray(a)
        if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1:
            raise ValueError("%s: %s must be (n >= 1, 3), got shape %s" % (name, what, a.shape))
        if a.dtype.kind not in "fiu":
            raise ValueError("%s: %s has dtype %s (numbers)" % (name, what, a.dtype))
        return np.ascontiguousarray(a, dtype=np.float32)

    xyz = points(xyz, "xyz")
    if normals is not None:
        normals = points(normals, "normals")
        if tuple(normals.shape) != tuple(xyz.shape):
            raise ValueError("%s: %s normals for %s points" % (name, tuple(normals.shape), tuple(xyz.shape)))
        if bool(getattr(xyz, "is_cuda", False)) != bool(getattr(normals, "is_cuda", False)):
            raise ValueError("%s: xyz and normals must be on the same side (both host arrays or both device tensors)" % name)
    if origin is not None:
        origin = np.ascontiguousarray(origin, dtype=np.float64)
        if origin.shape != (3,) or not np.all(np.isfinite(origin)):
            raise ValueError("%s: origin must be three finite numbers, got %r" % (name, origin))
    return xyz, normals, origin


MOST_POINTS = 2 ** 31 - 2 ** 20       # what the library's sorts and scans take


def _rows3(a, name, what):
    """An (n, 3) cloud for a standalone call: a torch device tensor as it is, anything else as a contiguous float32 array."""
    if hasattr(a, "data_ptr") and hasattr(a, "is_cuda"):          # torch tensor, without importing torch
        if a.dim() != 2 or a.shape[1] != 3 or "float32" not in str(a.dtype):
            raise ValueError("%s: %s must be (n, 3) float32, got %s %s" % (name, what, tuple(a.shape), a.dtype))
    else:
        a = np.asarray(a)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError("%s: %s must be (n, 3), got shape %s" % (name, what, a.shape))
        if a.dtype.kind not in "fiu":
            raise ValueError("%s: %s has dtype %s (numbers)" % (name, what, a.dtype))
        a = np.ascontiguousarray(a, dtype=np.float32)
    if not 1 <= a.shape[0] <= MOST_POINTS:
        raise ValueError("%s: %d rows of %s (1 .. 2^31 - 2^20)" % (name, a.shape[0], what))
    return a


def _whole(v, name, what, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        raise ValueError("%s: %s = %r (a whole number %s)" % (name, what, v, ">= %d" % lo if hi is None else "in %d .. %d" % (lo, hi)))
    return int(v)


def _sample_args(normals, m, grid=8, unoriented=False, seed=0, name="normal_space_sample"):
    """The arguments of a normal-space sample, checked before any call reaches the library: (normals, m, grid, unoriented, seed)."""
    normals = _rows3(normals, name, "normals")
    return (normals, _whole(m, name, "m", 1), _whole(grid, name, "grid", 1, 32), int(bool(unoriented)),
            _whole(seed, name, "seed", 0, 0xFFFFFFFF))


def _stability_args(xyz, normals, idx=None, name="stability"):
    """The arguments of a stability report, checked before any call reaches the library: (xyz, normals, idx or None)."""
    xyz, normals = _rows3(xyz, name, "xyz"), _rows3(normals, name, "normals")
    if tuple(normals.shape) != tuple(xyz.shape):
        raise ValueError("%s: %s normals for %s points" % (name, tuple(normals.shape), tuple(xyz.shape)))
    if bool(getattr(xyz, "is_cuda", False)) != bool(getattr(normals, "is_cuda", False)):
        raise ValueError("%s: xyz and normals must be on the same side (both host arrays or both device tensors)" % name)
    if idx is not None:
        idx = np.asarray(idx)
        if idx.ndim != 1 or idx.dtype.kind not in "iu" or not 1 <= len(idx) <= MOST_POINTS:
            raise ValueError("%s: idx must be a list of 1 .. 2^31 - 2^20 whole numbers" % name)
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        if idx.min() < 0 or idx.max() >= xyz.shape[0]:
            raise ValueError("%s: idx reaches outside 0 .. %d" % (name, xyz.shape[0] - 1))
    return xyz, normals, idx


ORIENT_SEEDS = {"keep": capi.OA_SEED_KEEP, "toward": capi.OA_SEED_TOWARD, "away": capi.OA_SEED_AWAY}


def _orient_args(k=8, max_dist=0.0, seed="away", point=None, normals=None, n=None, name="orient_target_normals"):
    """The arguments of a consistent orientation, checked before any call reaches the library: (k, max_dist, seed, point or None,
    normals or None).  n: the number of vertices, when it is known."""
    k = _whole(k, name, "k", 2, 64)
    if n is not None and k > n:
        raise ValueError("%s: k = %d for %d vertices (2 .. min(64, n))" % (name, k, n))
    if isinstance(max_dist, bool) or not isinstance(max_dist, (int, float, np.integer, np.floating)) or not 0 <= max_dist < float("inf"):
        raise ValueError("%s: max_dist = %r (finite and >= 0; 0: no cap)" % (name, max_dist))
    if isinstance(seed, str):
        if seed not in ORIENT_SEEDS:
            raise ValueError("%s: seed %r (use 'keep', 'toward' or 'away')" % (name, seed))
        seed = ORIENT_SEEDS[seed]
    elif isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed not in (0, 1, 2):
        raise ValueError("%s: seed %r (use 'keep', 'toward' or 'away')" % (name, seed))
    if point is not None:
        point = np.ascontiguousarray(point, dtype=np.float32)
        if point.shape != (3,) or not np.isfinite(point).all():
            raise ValueError("%s: point must be three finite numbers, got %r" % (name, point))
    elif seed == capi.OA_SEED_TOWARD:
        raise ValueError("%s: seed 'toward' needs a point" % name)
    if normals is not None:
        normals = np.asarray(normals)
        if normals.ndim != 2 or normals.shape[1] != 3 or normals.dtype.kind not in "fiu" or (n is not None and len(normals) != n):
            raise ValueError("%s: normals must be (%s, 3) numbers, got %s %s" % (name, "n" if n is None else n, normals.shape, normals.dtype))
        normals = np.ascontiguousarray(normals, dtype=np.float32)
    return k, float(max_dist), int(seed), point, normals


OUTLIER_METHODS = {"statistical": capi.OA_OUTLIER_STATISTICAL, "radius": capi.OA_OUTLIER_RADIUS}


def _real(v):
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def _outlier_args(method="statistical", k=16, std_ratio=2.0, radius=0.0, min_neighbors=8, count_cap=0, n=None,
                  name="target_outliers"):
    """The arguments of an outlier filter, checked before any call reaches the library: (method, k, std_ratio, radius,
    min_neighbors, count_cap), with the other method's fields left at values the library ignores.  n: the number of vertices,
    when it is known."""
    if isinstance(method, str):
        if method not in OUTLIER_METHODS:
            raise ValueError("%s: method %r (use 'statistical' or 'radius')" % (name, method))
        method = OUTLIER_METHODS[method]
    elif isinstance(method, bool) or not isinstance(method, (int, np.integer)) or method not in (0, 1):
        raise ValueError("%s: method %r (use 'statistical' or 'radius')" % (name, method))
    if method == capi.OA_OUTLIER_STATISTICAL:
        k = _whole(k, name, "k", 1, 63)
        if n is not None and k > n - 1:
            raise ValueError("%s: k = %d for %d vertices (1 .. min(63, n - 1))" % (name, k, n))
        if not _real(std_ratio) or not 0 <= std_ratio < float("inf"):
            raise ValueError("%s: std_ratio = %r (finite and >= 0)" % (name, std_ratio))
        return int(method), k, float(std_ratio), 0.0, 1, 0
    if not _real(radius) or not 0 < radius < float("inf"):
        raise ValueError("%s: radius = %r (finite and > 0)" % (name, radius))
    min_neighbors = _whole(min_neighbors, name, "min_neighbors", 1, 2**31 - 2)
    count_cap = _whole(count_cap, name, "count_cap", 0, 2**31 - 1)
    if count_cap != 0 and count_cap < min_neighbors + 1:
        raise ValueError("%s: count_cap = %d (0: exact counts, or >= min_neighbors + 1 = %d)" % (name, count_cap, min_neighbors + 1))
    return int(method), 1, 0.0, float(radius), min_neighbors, count_cap


def _radius_count_args(radius, cap=0, name="target_radius_count"):
    if not _real(radius) or not 0 < radius < float("inf"):
        raise ValueError("%s: radius = %r (finite and > 0)" % (name, radius))
    return float(radius), _whole(cap, name, "cap", 0, 2**31 - 1)


def _radius_arg(radius, name="set_neighbor_radius", what="radius", off_ok=False):
    """A neighbour radius, checked before any call reaches the library: a number, finite and > 0, that is still > 0 as a float32 and
    whose float32 square is finite (what the searches compare against).  off_ok: 0 is taken too and means "no limit".  Returns
    the float32 value as a float."""
    ok = _real(radius) and (radius > 0 or (off_ok and radius == 0))
    if ok and radius != 0:
        with np.errstate(over="ignore"):
            r = np.float32(radius)
            ok = bool(r > 0 and np.isfinite(r) and np.isfinite(r * r))
    if not ok:
        raise ValueError("%s: %s = %r (%sfinite and > 0, at most 1.8e19: its float32 square must be finite)"
                         % (name, what, radius, "0 = no limit, else " if off_ok else ""))
    return float(np.float32(radius))


CLUSTER_KEEP = {"clustered": capi.OA_CLUSTER_KEEP_CLUSTERED, "largest": capi.OA_CLUSTER_KEEP_LARGEST,
                "min_size": capi.OA_CLUSTER_KEEP_MIN_SIZE}


def _cluster_args(eps, min_points=8, keep="largest", min_size=0, name="target_clusters"):
    """The arguments of a clustering, checked before any call reaches the library: (eps, min_points, keep, min_size)."""
    if not _real(eps) or not 0 < eps < float("inf"):
        raise ValueError("%s: eps = %r (finite and > 0)" % (name, eps))
    min_points = _whole(min_points, name, "min_points", 1, 2**31 - 1)
    if isinstance(keep, str):
        if keep not in CLUSTER_KEEP:
            raise ValueError("%s: keep %r (use 'clustered', 'largest' or 'min_size')" % (name, keep))
        keep = CLUSTER_KEEP[keep]
    elif isinstance(keep, bool) or not isinstance(keep, (int, np.integer)) or keep not in (0, 1, 2):
        raise ValueError("%s: keep %r (use 'clustered', 'largest' or 'min_size')" % (name, keep))
    return float(eps), min_points, int(keep), _whole(min_size, name, "min_size", 0, 2**63 - 1)


DEVIATION_OUTPUTS = ("signed_d", "dist", "closest", "idx", "feature")
DEVIATION_SIGNED = {"auto": -1, "never": 0, "required": 1, None: -1, False: 0, True: 1}


def _deviation_args(thresh=float("inf"), signed="auto", quantiles=(0.5, 0.9, 0.95, 0.99), bins=0, hist_range=None,
                    outputs=("signed_d", "closest", "idx", "feature"), name="deviation"):
    """The arguments of a deviation report, checked before any call reaches the library: (thresh, signed_mode, quantiles, bins,
    (lo, hi), outputs)."""
    def number(v):
        return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))

    if not number(thresh) or np.isnan(thresh) or not thresh > 0:
        raise ValueError("%s: thresh = %r (> 0; inf counts every pair)" % (name, thresh))
    try:
        signed_mode = DEVIATION_SIGNED[signed]
    except (KeyError, TypeError):
        raise ValueError("%s: signed = %r (use 'auto', True / 'required' or False / 'never')" % (name, signed)) from None
    quantiles = tuple(quantiles) if quantiles is not None else ()
    if len(quantiles) > 8:
        raise ValueError("%s: %d quantiles (at most 8)" % (name, len(quantiles)))
    for q in quantiles:
        if not number(q) or not (q > 0 and q <= 1):
            raise ValueError("%s: quantile %r outside (0, 1]" % (name, q))
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 0 <= int(bins) <= 1024:
        raise ValueError("%s: bins = %r (0 .. 1024)" % (name, bins))
    lo, hi = 0.0, 0.0
    if hist_range is not None:
        try:
            lo, hi = hist_range
        except (TypeError, ValueError):
            raise ValueError("%s: hist_range = %r (lo, hi)" % (name, hist_range)) from None
        if not number(lo) or not number(hi) or not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise ValueError("%s: hist_range = %r (finite, lo < hi)" % (name, hist_range))
    elif int(bins) > 0:
        raise ValueError("%s: %d bins need a hist_range" % (name, int(bins)))
    if isinstance(outputs, str):
        outputs = (outputs,)
    outputs = tuple(outputs) if outputs is not None else ()
    for o in outputs:
        if o not in DEVIATION_OUTPUTS:
            raise ValueError("%s: unknown output %r (of %s)" % (name, o, ", ".join(DEVIATION_OUTPUTS)))
    return float(thresh), signed_mode, tuple(float(q) for q in quantiles), int(bins), (float(lo), float(hi)), outputs


def resolve_devices(spec):
    """A device list from an int, a sequence, "all", or a string like "0,1,2,3" (what OA_DEVICES may hold)."""
    if spec is None:
        return None
    if isinstance(spec, str):
        spec = spec.strip()
        if spec.lower() == "all":
            return list(range(device_count()))
        return [int(t) for t in spec.replace(";", ",").split(",") if t.strip() != ""]
    if isinstance(spec, (int, np.integer)):
        return [int(spec)]
    return [int(d) for d in spec]


class IcpEngine:
    """One context: one GPU (`device`, the HIP ordinal -- LOCAL_RANK in one-process-per-GPU runs), or several GPUs of
    this process (`devices=[0, 1, ...]`, oa_create_multi): the source is sharded over them, the target replicated,
    and run() / iterate() join the devices' sums inside the library every iteration.  `exchange`: "auto" (default:
    RCCL's all-reduce over xGMI when the devices are distinct and librccl loads, else the mailbox), "rccl" or
    "mailbox"."""

    def __init__(self, device: int = 0, devices=None, exchange=None, experiments: bool = False):
        # experiments: liboa_icp_exp.so -- the default library + the A/B predecessors and measured-but-not-kept variants
        # (csrc/oa_families.hpp); the OA_NN_SORT / OA_NN_MFMA / OA_TRI_RING / OA_GRID_STATS / OA_TRI_SHARE knobs only act there
        self._L = capi.load(experiments=experiments)
        h = C.c_void_p()
        devs = resolve_devices(devices)
        if devs is None:
            self._chk(self._L.oa_create(C.byref(h), int(device)))
            self.devices = [int(device)]
            self.multi = False
        else:
            arr = (C.c_int * len(devs))(*devs)
            self._chk(self._L.oa_create_multi(C.byref(h), arr, len(devs)))
            self.devices = devs
            self.multi = True
        self._h = h
        self.device = self.devices[0]
        self.n_target = 0
        self.n_selected = 0
        # who uploaded the geometry last (GpuBVH objects sharing one engine check these before they trust its state)
        self.target_owner = None
        self.source_owner = None
        if exchange is not None:
            self.set_exchange(exchange)

    def _chk(self, rc):
        return capi.check(rc, self._L)

    def set_exchange(self, mode):
        """'auto', 'rccl' (ncclAllReduce over xGMI) or 'mailbox' (all-gather through peer-mapped device mailboxes --
        pinned host memory without peer access --, rank-ordered sum)."""
        code = ({"auto": capi.OA_EXCHANGE_AUTO, "mailbox": capi.OA_EXCHANGE_MAILBOX, "rccl": capi.OA_EXCHANGE_RCCL}[mode]
                if isinstance(mode, str) else int(mode))
        self._chk(self._L.oa_set_exchange(self._h, code))

    # ---- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._L.oa_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, stream_handle):
        """stream_handle: integer hipStream_t, e.g. torch.cuda.current_stream().cuda_stream (0 = the legacy
        default stream); None = the context's private stream."""
        h = C.c_void_p(-1) if stream_handle is None else C.c_void_p(int(stream_handle))
        self._chk(self._L.oa_set_stream(self._h, h))

    def set_search_mode(self, mode):
        """'auto' (default), 'brute' (north-star LDS-tiled brute force), 'grid' (uniform-grid exact search, far
        queries finished by the tree) or 'bvh' (every query through the bounding-box tree).
        All modes return identical correspondences."""
        code = {"auto": -1, "brute": 0, "grid": 1, "bvh": 2}[mode] if isinstance(mode, str) else int(mode)
        self._chk(self._L.oa_set_search_mode(self._h, code))

    # ---- uploads
    def set_target(self, xyz):
        p, on_dev, keep, n = _device_ptr(xyz)
        self._chk(self._L.oa_set_target(self._h, p, n, on_dev))
        self.n_target = n
        self.target_owner = None
        del keep

    def set_target_mesh(self, xyz, tris):
        """Surface mode: closest point on the base mesh's triangles (BVHTree.find_nearest semantics).
        tris: (n, 3) vertex indices (triangulate quads/ngons first)."""
        p, on_dev, keep, n = _device_ptr(xyz)
        t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
        self._chk(self._L.oa_set_target_mesh(self._h, p, n, on_dev, t.ctypes.data_as(C.POINTER(C.c_int32)), len(t)))
        self.n_target = n
        self.target_owner = None
        del keep

    def set_source(self, xyz, vlist=None, stride=0, shard_index=0, shard_count=1):
        p, on_dev, keep, n = _device_ptr(xyz)
        if vlist is not None:
            vl = np.ascontiguousarray(vlist, dtype=np.int64)
            vp, nv = capi.iptr(vl), len(vl)
        else:
            vl, vp, nv = None, None, 0
        self._chk(self._L.oa_set_source(self._h, p, n, on_dev, vp, nv, int(stride), int(shard_index), int(shard_count)))
        self.n_selected = int(self._L.oa_num_selected(self._h))
        self.source_owner = None
        del keep, vl

    def set_normals(self, src_normals, tgt_normals=None, max_angle_deg=45.0):
        """Extension (not in the reference): drop pairs whose world-space normals differ by more than max_angle_deg.
        Call after set_source / set_target*; src_normals=None switches the test off."""
        if src_normals is None:
            self._chk(self._L.oa_set_normals(self._h, None, 0, None, 0, 0.0))
            return
        sn = capi.as_f32(src_normals).reshape(-1, 3)
        tn = capi.as_f32(tgt_normals).reshape(-1, 3) if tgt_normals is not None else None
        self._chk(self._L.oa_set_normals(self._h, capi.fptr(sn), len(sn), capi.fptr(tn) if tn is not None else None,
                                          len(tn) if tn is not None else 0, float(max_angle_deg)))

    METRICS = {"point": capi.OA_METRIC_POINT, "plane": capi.OA_METRIC_PLANE, "gicp": capi.OA_METRIC_GICP,
               "symmetric": capi.OA_METRIC_SYMMETRIC}

    def set_metric(self, metric):
        """What a loop step minimises: 'point' (Besl-McKay, the reference's loop, default), 'plane' (Chen-Medioni: the distance
        to the tangent plane at the correspondence) or 'gicp' (plane-to-plane, Generalized-ICP: every pair weighted by both sides'
        normals -- needs set_source_normals, see set_gicp) or 'symmetric' (Rusinkiewicz 2019: the plane metric's row with the mean
        of both sides' normals and the rotation split between the two sides -- needs set_source_normals, no parameter); the last
        three on single-device contexts, run() / iterate(), no scale.
        Survives uploads and set_matrices; stat("metric") reads it back."""
        if isinstance(metric, str):
            if metric not in self.METRICS:
                raise ValueError("metric %r (use 'point', 'plane', 'gicp' or 'symmetric')" % (metric,))
            metric = self.METRICS[metric]
        self._chk(self._L.oa_set_metric(self._h, int(metric)))

    def set_target_normals(self, tgt_normals):
        """Vertex-mode targets: one base-local normal per target vertex, for the plane metric (the normal-angle test stays as
        it is).  Call after set_target; a new target upload forgets them."""
        tn = capi.as_f32(tgt_normals).reshape(-1, 3)
        self._chk(self._L.oa_set_target_normals(self._h, capi.fptr(tn), len(tn)))

    def set_gicp(self, epsilon=1e-3):
        """The 'gicp' metric's epsilon: the small eigenvalue of each side's covariance I - (1 - epsilon) n n^T, in [1e-6, 1]
        (1e-3: the paper's; 1 makes the step the Gauss-Newton point-to-point one).  Survives uploads and set_matrices."""
        self._chk(self._L.oa_set_gicp(self._h, float(epsilon)))

    def set_source_normals(self, src_normals):
        """One align-local normal per source vertex (the array uploaded with set_source, not the selection), for the 'gicp'
        and 'symmetric' metrics; the normal-angle test stays as it is.  Call after set_source; a new source upload forgets them."""
        sn = capi.as_f32(src_normals).reshape(-1, 3)
        self._chk(self._L.oa_set_source_normals(self._h, capi.fptr(sn), len(sn)))

    ORIENTS = {"none": capi.OA_ORIENT_NONE, "toward": capi.OA_ORIENT_TOWARD, "away": capi.OA_ORIENT_AWAY}

    def set_neighbor_radius(self, radius):
        """Limit the neighbourhoods of target_knn, estimate_target_normals, target_fpfh and the cloud criterion of target_boundary
        / set_reject_boundary to the vertices within `radius` (the target's own units; the float32 metric against (float32
        radius)^2, as target_radius_count): rows are "the k nearest among those", shorter rows padded with -1 / +inf -- so that
        neighbours are not taken from the other side of a thin wall, the next tooth or across a hole.  0 or None: no limit (the
        default).  orient_target_normals (its own max_dist), the outlier, clustering and spacing calls do not look at it.
        Survives uploads and set_matrices; multi-device engines hand it to every child; neighbor_radius reads it back."""
        r = 0.0 if radius is None else _radius_arg(radius, off_ok=True)
        self._chk(self._L.oa_set_neighbor_radius(self._h, r))

    @property
    def neighbor_radius(self) -> float:
        """The neighbour radius in force (the float32 the library holds); 0.0 = no limit."""
        v = C.c_float(0.0)
        self._chk(self._L.oa_get_neighbor_radius(self._h, C.byref(v)))
        return float(v.value)

    @contextmanager
    def _radius_for(self, radius, name):
        """radius=None: the engine's own setting holds.  Else that radius (checked before the library is touched) for the calls
        inside, and the previous setting again behind them, refused calls included."""
        if radius is None:
            yield
            return
        r = _radius_arg(radius, name)
        prev = self.neighbor_radius
        self.set_neighbor_radius(r)
        try:
            yield
        finally:
            self.set_neighbor_radius(prev)

    def target_spacing(self):
        """Vertex-mode targets: the cloud's own point spacing -- {"mean", "std"} of the distance from every vertex to the nearest
        other vertex (a duplicate gives 0; fixed-order fp64 sums: two calls give the same bits), "n_finite" the vertices that
        have one and "n_nonfinite" the others (a non-finite coordinate).  What a neighbour radius, a voxel edge or an eps is a
        multiple of.  The neighbour radius does not apply.  Single-device contexts."""
        rep = capi.SpacingReport()
        self._chk(self._L.oa_target_spacing(self._h, C.byref(rep)))
        return {"mean": float(rep.mean), "std": float(rep.std), "n_finite": int(rep.n_finite), "n_nonfinite": int(rep.n_nonfinite)}

    def target_knn(self, k, radius=None):
        """Vertex-mode targets: the k nearest target vertices of every target vertex (itself included), exact and ordered by
        (d2, index): (idx int32 (nt, k), d2 float32 (nt, k)), in the caller's vertex order.  1 <= k <= min(64, nt).
        radius: this neighbour radius for the call (set_neighbor_radius; None: the engine's setting)."""
        r = None if radius is None else _radius_arg(radius, "target_knn")
        k = int(k)
        shape = (max(1, self.n_target), max(1, k))
        idx = np.empty(shape, np.int32)
        d2 = np.empty(shape, np.float32)
        with self._radius_for(r, "target_knn"):
            self._chk(self._L.oa_target_knn(self._h, k, idx.ctypes.data_as(C.POINTER(C.c_int32)), capi.fptr(d2)))
        return idx[: self.n_target], d2[: self.n_target]

    def estimate_target_normals(self, k=16, orient="none", orient_point=None, install=True, radius=None):
        """Vertex-mode targets: PCA normals from every vertex's k nearest neighbours, computed on the device: (normals float32
        (nt, 3), curvature float32 (nt,)).  orient: 'none' (canonical sign), 'toward' orient_point (a scanner position) or 'away'
        from it (an interior point; None = the target's centroid).  install: the normals become the target's (as after
        set_target_normals) without a host round trip.  Degenerate neighbourhoods give the zero normal.  3 <= k <= min(64, nt).
        radius: this neighbour radius for the call (set_neighbor_radius; None: the engine's setting); a vertex with fewer than
        three neighbours inside it gets the zero normal."""
        r = None if radius is None else _radius_arg(radius, "estimate_target_normals")
        if isinstance(orient, str):
            if orient not in self.ORIENTS:
                raise ValueError("orient %r (use 'none', 'toward' or 'away')" % (orient,))
            orient = self.ORIENTS[orient]
        pt = capi.as_f32(orient_point).reshape(3) if orient_point is not None else None
        nrm = np.empty((max(1, self.n_target), 3), np.float32)
        curv = np.empty(max(1, self.n_target), np.float32)
        with self._radius_for(r, "estimate_target_normals"):
            self._chk(self._L.oa_estimate_target_normals(self._h, int(k), int(orient), capi.fptr(pt) if pt is not None else None,
                                                          int(bool(install)), capi.fptr(nrm), capi.fptr(curv)))
        return nrm[: self.n_target], curv[: self.n_target]

    def orient_target_normals(self, k=8, max_dist=0.0, seed="away", point=None, normals=None, install=True):
        """Vertex-mode targets: one consistent sign for the cloud's normals, on the device (Hoppe et al. 1992): the minimum
        spanning forest of the k-nearest graph under the weights 1 - |n_i . n_j|, signs handed along its edges -- no view point
        needed, so a torus, an arch or a bent tube come out right where orient='away' cannot.  normals: (nt, 3), or None for
        the target's own (an installed estimate).  max_dist > 0 drops graph edges longer than that (a speck of noise then stays
        a component of its own).  seed: what fixes each component's overall sign -- 'keep' (its lowest vertex keeps its sign),
        'toward' point (its vertex nearest to point faces it) or 'away' from point (its farthest vertex faces away; None = the
        target's centroid).  Returns (normals float32 (nt, 3), flipped uint8 (nt,), component int32 (nt,) -- the lowest index of
        the vertex's component, -1 for a vertex without a usable normal --, report dict).  install: the result becomes the
        target's normals.  2 <= k <= min(64, nt)."""
        k, max_dist, seed, point, normals = _orient_args(k, max_dist, seed, point, normals, n=self.n_target or None)
        n = max(1, self.n_target)
        out = np.empty((n, 3), np.float32)
        flipped = np.empty(n, np.uint8)
        comp = np.empty(n, np.int32)
        rep = capi.OrientReport()
        self._chk(self._L.oa_orient_target_normals(self._h, k, max_dist, seed, capi.fptr(point) if point is not None else None,
                                                    capi.fptr(normals) if normals is not None else None, int(bool(install)),
                                                    capi.fptr(out), flipped.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                    comp.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(rep)))
        report = {name: int(getattr(rep, name)) for name, _ in capi.OrientReport._fields_ if name != "reserved"}
        return out[: self.n_target], flipped[: self.n_target], comp[: self.n_target], report

    def target_radius_count(self, radius, cap=0):
        """Vertex-mode targets: for every target vertex the number of target vertices within `radius` of it (the target's own
        units; the float32 metric against (float32 radius)^2), itself included: int32 (nt,).  cap > 0: counts saturate there
        and the search of a vertex stops when it is reached.  A vertex with a non-finite coordinate counts 0."""
        radius, cap = _radius_count_args(radius, cap)
        count = np.empty(max(1, self.n_target), np.int32)
        self._chk(self._L.oa_target_radius_count(self._h, radius, cap, count.ctypes.data_as(C.POINTER(C.c_int32))))
        return count[: self.n_target]

    def target_outliers(self, method="statistical", k=16, std_ratio=2.0, radius=0.0, min_neighbors=8, count_cap=0, apply=False):
        """Vertex-mode targets: which vertices are stray points.  method 'statistical': a vertex stays when the mean distance to
        its k nearest other vertices is at most mean + std_ratio * std of that figure over the cloud; 'radius': when at least
        min_neighbors other vertices lie within `radius` (the target's own units; count_cap > 0 lets the counts saturate there).
        Returns {"keep": uint8 (nt,), "score": float64 (nt,) or "count": int32 (nt,), "index": int32 (n_kept,) -- the kept vertices,
        ascending --, "report": dict}.  apply: the kept vertices become the target, exactly as set_target(xyz[keep]) would make
        them (normals, descriptors and boundary masks of the old target are forgotten); stat("target_cleaned") then holds the
        number removed."""
        method, k, std_ratio, radius, min_neighbors, count_cap = _outlier_args(method, k, std_ratio, radius, min_neighbors, count_cap,
                                                                                 n=self.n_target or None)
        n = max(1, self.n_target)
        st = capi.OutlierSettings(method, k, std_ratio, radius, min_neighbors, count_cap)
        rep = capi.OutlierReport()
        keep = np.empty(n, np.uint8)
        index = np.empty(n, np.int32)
        statistical = method == capi.OA_OUTLIER_STATISTICAL
        score = np.empty(n, np.float64) if statistical else None
        count = None if statistical else np.empty(n, np.int32)
        i32p = C.POINTER(C.c_int32)
        nt = self.n_target
        self._chk(self._L.oa_target_outliers(self._h, C.byref(st), int(bool(apply)), keep.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             capi.dptr(score) if statistical else None, None if statistical else count.ctypes.data_as(i32p),
                                             index.ctypes.data_as(i32p), C.byref(rep)))
        report = {name: (int if name.startswith("n_") else float)(getattr(rep, name)) for name, _ in capi.OutlierReport._fields_}
        out = {"keep": keep[:nt], "index": index[: report["n_kept"]].copy(), "report": report}
        out["score" if statistical else "count"] = (score if statistical else count)[:nt]
        if apply:
            self.n_target = report["n_kept"]
            self.target_owner = None
        return out

    def target_clusters(self, eps, min_points=8, keep="largest", min_size=0, apply=False):
        """Vertex-mode targets: the parts of the cloud, by DBSCAN (the answer scikit-learn's DBSCAN(algorithm="brute") gives, its
        numbering and border assignment included).  A vertex with at least min_points vertices within eps (the target's own units;
        itself included) is a core vertex; core vertices within eps of each other share a cluster, clusters are numbered by their
        lowest core index; a non-core vertex within eps of a core vertex takes the lowest such cluster's label; the rest is noise,
        -1.  keep: 'clustered' (label >= 0), 'largest' (the largest cluster; on equal size the lowest label) or 'min_size' (clusters
        of at least min_size members).  Returns {"label": int32 (nt,), "sizes": int32 (n_clusters,), "keep": uint8 (nt,), "index":
        int32 (n_kept,) -- the kept vertices, ascending --, "report": dict}.  apply: the kept vertices become the target, exactly as
        set_target(xyz[keep]) would make them; stat("target_cleaned") then holds the number removed."""
        eps, min_points, keep, min_size = _cluster_args(eps, min_points, keep, min_size)
        nt = self.n_target
        n = max(1, nt)
        st = capi.ClusterSettings(eps, min_points, keep, min_size)
        rep = capi.ClusterReport()
        label, sizes, index = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
        mask = np.empty(n, np.uint8)
        i32p = C.POINTER(C.c_int32)
        rc = self._L.oa_target_clusters(self._h, C.byref(st), int(bool(apply)), label.ctypes.data_as(i32p), sizes.ctypes.data_as(i32p),
                                        mask.ctypes.data_as(C.POINTER(C.c_uint8)), index.ctypes.data_as(i32p), C.byref(rep))
        self._chk(rc)
        report = {name: int(getattr(rep, name)) for name, _ in capi.ClusterReport._fields_}
        out = {"label": label[:nt], "sizes": sizes[: report["n_clusters"]].copy(), "keep": mask[:nt],
               "index": index[: report["n_kept"]].copy(), "report": report}
        if apply:
            self.n_target = report["n_kept"]
            self.target_owner = None
        return out

    LOSSES = {"none": capi.OA_LOSS_NONE, "huber": capi.OA_LOSS_HUBER, "tukey": capi.OA_LOSS_TUKEY, "cauchy": capi.OA_LOSS_CAUCHY}

    def set_robust(self, loss, scale=0.0):
        """Weight every pair of a loop step by a robust loss of its residual: 'none' (default), 'huber', 'tukey' or 'cauchy' (or
        the OA_LOSS_* integer), with the fixed scale `scale` in world units, like thresh.  The residual is the pair distance
        (point metric) or the distance to the tangent plane (plane metric).  K and mean / std distance stay unweighted.
        Survives uploads and set_matrices; stat("robust_loss") reads it back, stat("weight_sum") the last step's sum of weights."""
        if isinstance(loss, str):
            if loss not in self.LOSSES:
                raise ValueError("loss %r (use 'none', 'huber', 'tukey' or 'cauchy')" % (loss,))
            loss = self.LOSSES[loss]
        self._chk(self._L.oa_set_robust(self._h, int(loss), float(scale)))

    def set_robust_auto(self, quantile=0.0, scale_min=0.0):
        """Take the loss's scale from each step's own residuals: c = max(scale * q, scale_min), q the ceil(quantile * K_q)-th
        smallest float32 residual of the step's pairs (those of vertex weight 0 left out) and `scale` the multiplier given to
        set_robust -- quantile 0.5 with 1.4826 x the loss's tuning constant is the MAD scale.  scale_min (world units, > 0) keeps
        c off zero on exact data.  quantile 0 (default) switches it off; inert while the loss is 'none'.  Single-device
        contexts, run / iterate only.  stat("robust_scale") reads the last step's c back, stat("robust_quantile") the setting."""
        self._chk(self._L.oa_set_robust_auto(self._h, float(quantile), float(scale_min)))

    def set_reciprocal(self, on=True, ratio=1.0):
        """Keep a pair of a step only if it is mutual: the source point must also be the nearest selected source point of its
        own correspondence (ratio 1, ties kept), or within `ratio` times that nearest distance (ratio in [1, 16]).  What a whole
        model against a partial scan needs: the source points outside the overlap pair with the target's rim, and those pairs
        are not mutual.  Applies to run / iterate / make_pairs on single-device engines that hold the whole selection; nn_search,
        deviation, score_poses and coarse_align do not look at it.  Survives uploads and set_matrices; stat("reciprocal") /
        stat("reciprocal_ratio") read it back, stat("recip_rejected") the pairs the last step dropped for it."""
        self._chk(self._L.oa_set_reciprocal(self._h, int(bool(on)), float(ratio)))

    def set_trim(self, fraction=0.0, fraction_min=0.3, lam=2.0):
        """Trimmed ICP: every step keeps only the pairs with the smallest residuals.  fraction: 0 = off, a share in (0, 1] (the
        overlap of the two clouds), or "auto": every step estimates the share itself (fractional ICP: the share that minimises
        FRMSD with exponent `lam`, searched from fraction_min up).  Needs no scale in world units and no tree over the source, and
        drops displaced outliers as well as the rim of an overlap.  Applies to run / iterate / make_pairs on single-device engines
        that hold the whole selection; nn_search, deviation, score_poses and coarse_align do not look at it.  Survives uploads and
        set_matrices; stat("trim") reads the setting back (-1: auto), stat("trim_candidates") / stat("trim_kept") /
        stat("trim_cut") the last step's candidates, survivors and cut."""
        if isinstance(fraction, str):
            if fraction != "auto":
                raise ValueError('fraction must be a number or "auto"')
            fraction = capi.OA_TRIM_AUTO
        self._chk(self._L.oa_set_trim(self._h, float(fraction), float(fraction_min), float(lam)))

    def set_reject_boundary(self, on=True, k=16, angle_deg=90.0):
        """Drop a pair of a step whose correspondence lies on the target's boundary (target_boundary's masks, built before the
        loop starts): on a mesh target the closest point lies on an edge only one triangle owns, or on an end of one; on a cloud
        target the winning vertex is flagged by the angle criterion (k, angle_deg; the target needs its normals).  What a whole
        model against a partial scan needs: the source points outside the overlap pair with the target's rim.  Applies to run /
        iterate / make_pairs on single-device engines that hold the whole selection; nn_search, deviation, score_poses and
        coarse_align do not look at it.  Survives uploads and set_matrices; stat("reject_boundary") reads it back,
        stat("boundary_rejected") the pairs the last step dropped for it."""
        self._chk(self._L.oa_set_reject_boundary(self._h, int(bool(on)), int(k), float(angle_deg)))

    def target_boundary(self, k=16, angle_deg=90.0, radius=None):
        """The boundary of the resident target, built on the device if it is not there yet: (vertex_mask uint8 (n_verts,),
        edge_mask uint8 (n_tris,) or None).  Mesh targets: exact -- bit j of edge_mask[t] = local edge j (ab, bc, ca) of triangle
        t belongs to exactly one triangle; vertex_mask = the ends of such edges; k and angle_deg are ignored.  Cloud targets (with
        normals installed): vertex_mask by the angle criterion -- the largest gap between the tangent-plane directions to the k
        nearest neighbours exceeds angle_deg -- and edge_mask is None.  3 <= k <= min(63, nt - 1), 0 < angle_deg < 360.
        stat("target_boundary") / stat("boundary_vertices") / stat("boundary_edges") describe the built masks.
        radius (cloud targets): this neighbour radius for the call (set_neighbor_radius; None: the engine's setting) -- the k
        nearest no longer reach across a hole narrower than their spread; fewer than three neighbours inside it: on the rim."""
        r = None if radius is None else _radius_arg(radius, "target_boundary")
        u8 = C.POINTER(C.c_uint8)
        vm = np.empty(max(1, self.n_target), np.uint8)
        n_tris = int(self.stat("n_tris")) if int(self.stat("surface")) else 0
        em = np.empty(max(1, n_tris), np.uint8) if n_tris > 0 else None
        with self._radius_for(r, "target_boundary"):
            self._chk(self._L.oa_target_boundary(self._h, int(k), float(angle_deg), vm.ctypes.data_as(u8),
                                                 em.ctypes.data_as(u8) if em is not None else None))
        return vm[: self.n_target], (em[:n_tris] if em is not None else None)

    def set_source_weights(self, weights):
        """One weight per source vertex (finite, >= 0; the array uploaded with set_source, not the selection): a pair's weight
        is this times the robust loss's.  None switches them off; a new set_source forgets them.  Call after set_source."""
        if weights is None:
            self._chk(self._L.oa_set_source_weights(self._h, None, 0))
            return
        w = capi.as_f32(weights).reshape(-1)
        self._chk(self._L.oa_set_source_weights(self._h, capi.fptr(w), len(w)))

    def set_matrices(self, mx_align, mx_base):
        a, b = capi.as_f32(mx_align, (4, 4)), capi.as_f32(mx_base, (4, 4))
        self._chk(self._L.oa_set_matrices(self._h, capi.fptr(a), capi.fptr(b)))

    def reset_seeds(self):
        """Forget the previous searches' answers (the next search starts cold; results are unaffected)."""
        self._chk(self._L.oa_reset_seeds(self._h))

    STATS = {"grid_cells": 1, "tri_grid_cells": 2, "tri_grid_entries": 3, "n_tris": 4, "surface": 5, "cache_bytes": 6,
             "brute_kernel": 7, "exchange": 8, "rccl_ranks": 9, "enqueue_us": 10, "host_threads": 11,
             "fast_iterations": 12, "handover_entries": 13, "handover_wave_max": 14, "enqueued_min": 15, "enqueued_max": 16,
             "watchdog_aborts": 17, "nn_ms_min": 18, "nn_ms_max": 19, "safe_radii": 20,
             "tri_ring": 21, "tri_ring_accepts": 22, "exchange_us": 23, "rccl_fallbacks": 24, "rccl_ranks_last": 25, "search_clock_mhz": 26, "brute_queue_wgs": 27,
             "metric": 28, "plane_rank": 29, "robust_loss": 30, "weight_sum": 31,
             "robust_scale": 32, "robust_quantile": 33, "target_normals": 34,
             "target_features": 35, "mesh_pseudonormals": 36,
             "reciprocal": 37, "reciprocal_ratio": 38, "recip_rejected": 39,
             "trim": 40, "trim_candidates": 41, "trim_kept": 42, "trim_cut": 43,
             "reject_boundary": 44, "boundary_rejected": 45, "target_boundary": 46, "boundary_vertices": 47, "boundary_edges": 48,
             "acc_path": 49, "acc_rows": 50, "target_cleaned": 51}
    EXCHANGE_NAMES = {-1: None, 0: "mailbox (pinned host memory)", 1: "rccl", 2: "mailbox (peer-mapped device memory)"}

    def exchange_info(self):
        """What a multi-device engine's loops exchange their sums through: {"exchange": name, "rccl_ranks": n}."""
        note = self._L.oa_exchange_note(self._h)
        return {"exchange": self.EXCHANGE_NAMES.get(int(self.stat("exchange"))), "rccl_ranks": int(self.stat("rccl_ranks")),
                "host_threads": int(self.stat("host_threads")), "note": note.decode("utf-8", "replace") if note else "",
                "rccl_ranks_last": int(self.stat("rccl_ranks_last")), "rccl_fallbacks": int(self.stat("rccl_fallbacks"))}

    def stat(self, name) -> float:
        v = C.c_double(0.0)
        self._chk(self._L.oa_get_stat(self._h, self.STATS[name] if isinstance(name, str) else int(name), C.byref(v)))
        return float(v.value)

    def search_ms(self, max_n=1 << 16) -> np.ndarray:
        """Search time (ms) of every iteration of the last run (oa_get_search_ms)."""
        out = np.zeros(int(max_n), np.float64)
        n = self._L.oa_get_search_ms(self._h, int(max_n), capi.dptr(out))
        if n < 0:
            self._chk(n)
        return out[:n].copy()

    def valu_ceiling(self, target_ms=5.0) -> dict:
        """What the vector ALUs issue right now (oa_measure_valu_ceiling): v_add_f32 (the issue rate) and v_min3_f32 (the half-rate class) on every SIMD."""
        out = np.zeros(4, np.float64)
        self._chk(self._L.oa_measure_valu_ceiling(self._h, float(target_ms), capi.dptr(out)))
        return {"tlaneops": float(out[0]), "shader_clock_mhz": float(out[1]), "ms": float(out[2]), "tlaneops_min3": float(out[3])}

    def enqueued_iterations(self):
        """Iterations the host enqueued for every child in the last run() (OA_STAT_ENQUEUED_CHILD + i): all equal, whatever
        the host threads saw of their devices while they enqueued (docs/HISTORY.md 4.7)."""
        return [int(self.stat(1000 + i)) for i in range(len(self.devices))] if self.multi else [int(self.stat("enqueued_max"))]

    def matrix_world(self) -> np.ndarray:
        out = np.empty((4, 4), np.float32)
        self._chk(self._L.oa_get_matrix_world(self._h, capi.fptr(out)))
        return out

    def pivot(self) -> np.ndarray:
        out = np.empty(3, np.float64)
        self._chk(self._L.oa_get_pivot(self._h, capi.dptr(out)))
        return out

    # ---- contract 1
    def make_pairs(self, thresh, calc_stats=False):
        cap = max(1, self.n_selected)
        A = np.zeros((3, cap), np.float64)
        B = np.zeros((3, cap), np.float64)
        K = C.c_int64(0)
        ds = np.zeros(2, np.float64)
        self._chk(self._L.oa_make_pairs(self._h, float(thresh), int(bool(calc_stats)), capi.dptr(A), capi.dptr(B),
                                         cap, C.byref(K), capi.dptr(ds)))
        k = int(K.value)
        d_stats = [float(ds[0]), float(ds[1])] if calc_stats else None
        return np.ascontiguousarray(A[:, :k]), np.ascontiguousarray(B[:, :k]), d_stats

    def nn_search(self, want_output=True):
        """Nearest target vertex per selected source point: (idx int64[n], d2 float32[n], kernel_ms)."""
        ms = C.c_double(0.0)
        if want_output:
            idx = np.empty(max(1, self.n_selected), np.int64)
            d2 = np.empty(max(1, self.n_selected), np.float32)
            self._chk(self._L.oa_nn_search(self._h, capi.iptr(idx), capi.fptr(d2), C.byref(ms)))
            return idx[: self.n_selected], d2[: self.n_selected], float(ms.value)
        self._chk(self._L.oa_nn_search(self._h, None, None, C.byref(ms)))
        return None, None, float(ms.value)

    # ---- contract 2
    def kabsch(self, A, B, scale=False, horn=False) -> np.ndarray:
        """horn: the rotation through Horn's quaternion (the reference's usesvd=False branch, functions/general.py:191-206)
        instead of the SVD of the covariance -- the same optimum, another route to it."""
        A = np.ascontiguousarray(A, np.float64)
        B = np.ascontiguousarray(B, np.float64)
        M = np.empty((4, 4), np.float64)
        rc = self._L.oa_kabsch(self._h, capi.dptr(A), capi.dptr(B), A.shape[1], A.shape[1], int(bool(scale)) | (2 if horn else 0), capi.dptr(M))
        if rc == capi.OA_E_TOO_FEW_PAIRS:
            raise ValueError(REF_VALUEERROR)
        self._chk(rc)
        return M

    def affine_from_points(self, v0, v1, shear=True, scale=True) -> np.ndarray:
        """affine_matrix_from_points in full: any ndims in 2..64, shear (affine) or rigid / similarity."""
        v0 = np.ascontiguousarray(v0, np.float64)
        v1 = np.ascontiguousarray(v1, np.float64)
        n, K = v0.shape
        M = np.empty((n + 1, n + 1), np.float64)
        rc = self._L.oa_affine_from_points(self._h, capi.dptr(v0), capi.dptr(v1), n, K, K, int(bool(shear)), int(bool(scale)),
                                           capi.dptr(M))
        if rc == capi.OA_E_TOO_FEW_PAIRS:
            raise ValueError(REF_VALUEERROR)
        self._chk(rc)
        return M

    def kabsch_from_sums(self, sums, pivot=None, scale=False) -> np.ndarray:
        s = np.ascontiguousarray(sums, np.float64).reshape(capi.OA_NSUMS)
        pv = np.ascontiguousarray(pivot, np.float64).reshape(3) if pivot is not None else None
        M = np.empty((4, 4), np.float64)
        rc = self._L.oa_kabsch_from_sums(self._h, capi.dptr(s), capi.dptr(pv) if pv is not None else None,
                                         int(bool(scale)), capi.dptr(M))
        if rc == capi.OA_E_TOO_FEW_PAIRS:
            raise ValueError(REF_VALUEERROR)
        self._chk(rc)
        return M

    def point_to_plane(self, A, B, N) -> np.ndarray:
        """The plane step from explicit pairs (3 x K each; N: the correspondences' normals, any length): the 4 x 4 that moves A
        towards the tangent planes at B, about the pivot A[:, 0]; minimum-norm where the pairs leave the step undetermined
        (stat("plane_rank") says how many directions they fix)."""
        A = np.ascontiguousarray(A, np.float64)
        B = np.ascontiguousarray(B, np.float64)
        N = np.ascontiguousarray(N, np.float64)
        if A.ndim != 2 or A.shape[0] != 3 or B.shape != A.shape or N.shape != A.shape:
            raise ValueError(REF_VALUEERROR)
        M = np.empty((4, 4), np.float64)
        rc = self._L.oa_point_to_plane(self._h, capi.dptr(A), capi.dptr(B), capi.dptr(N), A.shape[1], A.shape[1], capi.dptr(M))
        if rc == capi.OA_E_TOO_FEW_PAIRS:
            raise ValueError(REF_VALUEERROR)
        self._chk(rc)
        return M

    def symmetric_step(self, A, B, NA, NB) -> np.ndarray:
        """The symmetric metric's step from explicit pairs (3 x K each; NA, NB: the normals at A and at B, any length, either
        sign): the 4 x 4 that moves A towards B about the pivot A[:, 0], half of its rotation on either side of the translation;
        minimum-norm where the pairs leave the step undetermined (stat("plane_rank")).  A pair with a zero normal is left out."""
        A, B, NA, NB = (np.ascontiguousarray(x, np.float64) for x in (A, B, NA, NB))
        if A.ndim != 2 or A.shape[0] != 3 or B.shape != A.shape or NA.shape != A.shape or NB.shape != A.shape:
            raise ValueError(REF_VALUEERROR)
        M = np.empty((4, 4), np.float64)
        rc = self._L.oa_symmetric_step(self._h, capi.dptr(A), capi.dptr(B), capi.dptr(NA), capi.dptr(NB), A.shape[1], A.shape[1], capi.dptr(M))
        if rc == capi.OA_E_TOO_FEW_PAIRS:
            raise ValueError(REF_VALUEERROR)
        self._chk(rc)
        return M

    # ---- the loop
    @staticmethod
    def _settings(iters, thresh, target_d, use_target, with_scale, early_exit):
        return capi.Settings(int(iters), int(bool(use_target)), int(bool(with_scale)), int(bool(early_exit)),
                             float(thresh), float(target_d))

    def _history(self, n):
        n = max(0, int(n))
        m = max(1, n)
        sM = np.zeros((m, 4, 4), np.float64)
        sN = np.zeros((m, 4, 4), np.float32)
        sK = np.zeros(m, np.int64)
        sS = np.zeros((m, 2), np.float64)
        sT = np.zeros(m, np.float64)
        got = self._L.oa_get_history(self._h, m, capi.dptr(sM), capi.fptr(sN), capi.iptr(sK), capi.dptr(sS), capi.dptr(sT))
        got = max(0, min(int(got), n))
        return sM[:got], sN[:got], sK[:got], sS[:got], sT[:got]

    def _result(self, rep) -> RunResult:
        sM, sN, sK, sS, sT = self._history(rep.iters_done)
        return RunResult(rep.iters_done, bool(rep.converged), self.matrix_world(), int(rep.last_K),
                         rep.last_translation, rep.mean_dist, rep.std_dist, rep.mean_rot_angle, rep.nn_ms_total,
                         rep.loop_ms, sM, sN, sK, sS, sT)

    def run(self, iters=50, thresh=0.5, target_d=0.01, use_target=True, with_scale=False, early_exit=True) -> RunResult:
        st = self._settings(iters, thresh, target_d, use_target, with_scale, early_exit)
        rep = capi.Report()
        rc = self._L.oa_run(self._h, C.byref(st), C.byref(rep))
        if rc == capi.OA_E_TOO_FEW_PAIRS:
            # the reference raises out of affine_matrix_from_points in iteration n, after iterations 0..n-1 have been
            # applied to the objects (operators/icp_align.py:121-127): the partial result travels with the exception
            err = ValueError(REF_VALUEERROR)
            try:
                err.partial = self._result(rep)
            except Exception:
                err.partial = None
            raise err
        self._chk(rc)
        return self._result(rep)

    def iterate(self, thresh=0.5, target_d=0.01, use_target=True, with_scale=False):
        """One iteration (modal operator step).  Returns (M float64 4x4, stats dict)."""
        st = self._settings(1, thresh, target_d, use_target, with_scale, False)
        M = np.empty((4, 4), np.float64)
        s = np.empty(6, np.float64)
        rc = self._L.oa_iterate(self._h, C.byref(st), capi.dptr(M), capi.dptr(s))
        if rc == capi.OA_E_TOO_FEW_PAIRS:
            raise ValueError(REF_VALUEERROR)
        self._chk(rc)
        return M, dict(K=int(s[0]), mean_dist=s[1], std_dist=s[2], translation=s[3], rot_angle=s[4],
                       converged=bool(s[5]))

    # ---- coarse global alignment (extension; single-device contexts)
    def score_poses(self, mx_align_list, thresh, stride=1) -> np.ndarray:
        """Scores of P candidate align matrices in one launch: (P, 4) float64 [K, mean_dist, std_dist, cost] per pose over the
        selection's points at positions 0, stride, 2 stride, ... -- K / mean / std are what make_pairs(thresh, calc_stats=True)
        reports for that pose and sample, cost is the mean of min(dist, thresh) (lower is better).  No side effects."""
        m = capi.as_f32(mx_align_list).reshape(-1, 4, 4)
        out = np.empty((max(1, len(m)), capi.OA_POSE_NSCORE), np.float64)
        self._chk(self._L.oa_score_poses(self._h, capi.fptr(m), len(m), float(thresh), int(stride), capi.dptr(out)))
        return out[: len(m)]

    def coarse_candidates(self, n_rot) -> np.ndarray:
        """(n_rot, 4, 4) float32 align matrices: the current matrix_world turned about the selection's world centroid by the
        n_rot-point super-Fibonacci rotations, its centroid moved onto the target's.  No side effects."""
        n = int(n_rot)
        out = np.empty((max(1, n), 4, 4), np.float32)
        self._chk(self._L.oa_coarse_candidates(self._h, n, capi.fptr(out)))
        return out[:n]

    def coarse_align(self, thresh, n_rot=256, n_refine=8, refine_iters=10, stride=4) -> dict:
        """Multi-start: score n_rot candidates and the current pose, refine the n_refine cheapest for refine_iters point
        iterations over the sample, make the cheapest matrix_world (the current pose stays when nothing beats it).  Returns the
        report as a dict, with the new "matrix_world"."""
        cs = capi.CoarseSettings(int(n_rot), int(n_refine), int(refine_iters), int(stride), float(thresh))
        rep = capi.CoarseReport()
        self._chk(self._L.oa_coarse_align(self._h, C.byref(cs), C.byref(rep)))
        out = {name: getattr(rep, name) for name, _ in capi.CoarseReport._fields_}
        out["matrix_world"] = self.matrix_world()
        return out

    def coarse_align_poses(self, mx_align_list, thresh, n_refine=8, refine_iters=10, stride=4) -> dict:
        """coarse_align's recipe over caller-supplied candidates (P x 4 x 4) instead of the rotation set: score them and the
        current pose, refine the n_refine cheapest, make the cheapest matrix_world.  Returns the report as a dict, with the new
        "matrix_world"; best_candidate == P names the incoming pose."""
        m = capi.as_f32(mx_align_list).reshape(-1, 4, 4)
        cs = capi.CoarseSettings(0, int(n_refine), int(refine_iters), int(stride), float(thresh))
        rep = capi.CoarseReport()
        self._chk(self._L.oa_coarse_align_poses(self._h, capi.fptr(m), len(m), C.byref(cs), C.byref(rep)))
        out = {name: getattr(rep, name) for name, _ in capi.CoarseReport._fields_}
        out["matrix_world"] = self.matrix_world()
        return out

    def target_fpfh(self, k=16, keep=True, radius=None):
        """Vertex-mode targets with normals: the Fast Point Feature Histogram of every target vertex from its k nearest
        neighbours, (nt, 33) float32; an all-zero row means "no descriptor".  keep: the descriptors stay on the device for
        feature_candidates(tgt_feat=None) until the next set_target.  4 <= k <= min(64, nt).
        radius: this neighbour radius for the call (set_neighbor_radius; None: the engine's setting)."""
        k = _fpfh_k(k)
        r = None if radius is None else _radius_arg(radius, "target_fpfh")
        out = np.empty((max(1, self.n_target), capi.OA_FPFH_DIM), np.float32)
        with self._radius_for(r, "target_fpfh"):
            self._chk(self._L.oa_target_fpfh(self._h, k, capi.fptr(out), int(bool(keep))))
        return out[: self.n_target]

    def match_features(self, fa, fb):
        """Nearest rows in descriptor space: for every row of fa (na, dim) the row of fb (nb, dim) at the smallest squared L2
        distance: (idx int32 (na,), d2 float32 (na,), d2_second float32 (na,)).  Ties go to the lowest index; all-zero rows mean
        "no descriptor" and neither query nor answer (index -1, +inf).  1 <= dim <= 64."""
        fa, fb = _feature_rows(fa, "fa"), _feature_rows(fb, "fb")
        if fa.shape[1] != fb.shape[1]:
            raise ValueError("match_features: rows of %d and of %d floats" % (fa.shape[1], fb.shape[1]))
        idx = np.empty(len(fa), np.int32)
        d2 = np.empty(len(fa), np.float32)
        sec = np.empty(len(fa), np.float32)
        self._chk(self._L.oa_match_features(self._h, capi.fptr(fa), len(fa), capi.fptr(fb), len(fb), fa.shape[1],
                                            idx.ctypes.data_as(C.POINTER(C.c_int32)), capi.fptr(d2), capi.fptr(sec)))
        return idx, d2, sec

    def feature_candidates(self, src_feat, tgt_feat=None, n_hyp=4096, ratio=0.9, mutual=True, edge_tol=0.9, min_edge=0.0, seed=0,
                           triples=None):
        """Candidate align matrices from matched descriptors: src_feat (one row per SOURCE VERTEX, as set_source_normals takes
        its rows), tgt_feat (one row per target vertex; None: what target_fpfh(keep=True) left on the device).  Pairs that are mutual nearest rows and pass the ratio test (mutual
        False: the ratio test alone), ordered by source vertex; n_hyp triples of them (`triples`, (n_hyp, 3) pair indices, or a
        hashed draw from `seed`); every triple whose edge lengths agree within edge_tol and exceed min_edge (0: 5 % of the
        target's diagonal) gives the rigid motion of its three pairs.  Returns ((n, 4, 4) float32, report dict); n may be 0."""
        src_feat = _feature_rows(src_feat, "src_feat")
        if tgt_feat is not None:
            tgt_feat = _feature_rows(tgt_feat, "tgt_feat")
            if src_feat.shape[1] != tgt_feat.shape[1]:
                raise ValueError("feature_candidates: rows of %d and of %d floats" % (src_feat.shape[1], tgt_feat.shape[1]))
            if tgt_feat.shape[0] != self.n_target:
                raise ValueError("feature_candidates: %d descriptor rows for %d target vertices" % (tgt_feat.shape[0], self.n_target))
        tri = None
        if triples is not None:
            tri = np.ascontiguousarray(triples, dtype=np.int32)
            if tri.ndim != 2 or tri.shape[1] != 3 or len(tri) < 1:
                raise ValueError("feature_candidates: triples must be (n_hyp, 3) pair indices")
            n_hyp = len(tri)
        n_hyp = int(n_hyp)
        if not 1 <= n_hyp <= 65535:
            raise ValueError("feature_candidates: n_hyp %d outside 1 .. 65535" % n_hyp)
        fs = capi.FeatureSettings(src_feat.shape[1], n_hyp, int(bool(mutual)), int(seed) & 0xFFFFFFFF, float(ratio), float(edge_tol),
                                  float(min_edge))
        rep = capi.FeatureReport()
        out = np.empty((n_hyp, 4, 4), np.float32)
        n = C.c_int32(0)
        self._chk(self._L.oa_feature_candidates(self._h, capi.fptr(src_feat), len(src_feat), capi.fptr(tgt_feat) if tgt_feat is not None else None, C.byref(fs),
                                                tri.ctypes.data_as(C.POINTER(C.c_int32)) if tri is not None else None,
                                                capi.fptr(out), C.byref(n), C.byref(rep)))
        return out[: n.value].copy(), {name: getattr(rep, name) for name, _ in capi.FeatureReport._fields_ if name != "reserved"}

    def voxel_downsample(self, xyz, voxel, normals=None, origin=None):
        """Voxel-grid downsample of ANY cloud (no target, source or matrices needed; nothing a loop reads is touched): one row per
        occupied cell of edge `voxel`, in ascending cell order.  xyz / normals: (n, 3) host arrays or torch device tensors;
        origin: the grid's corner, None = the minimum of the finite points.  Returns a dict: xyz float32 (m, 3) the members'
        means, normals float32 (m, 3) the normalised sums of their normals (None without normals), count int32 (m,), rep int64
        (m,) the index of the member nearest to each mean (what makes a downsample a vlist), report."""
        xyz, normals, origin = _voxel_args(xyz, voxel, normals, origin)
        p, on_dev, keep, n = _device_ptr(xyz)
        pn, keep_n = None, None
        if normals is not None:
            pn, _, keep_n, _ = _device_ptr(normals)
        rep = capi.VoxelReport()
        m = C.c_int64(0)
        i32p = C.POINTER(C.c_int32)
        po = capi.dptr(origin) if origin is not None else None
        # room for the most rows there can be (untouched pages cost nothing; the library copies n_voxels rows)
        out = np.empty((n, 3), np.float32)
        out_n = np.empty((n, 3), np.float32) if normals is not None else None
        cnt = np.empty(n, np.int32)
        idx = np.empty(n, np.int64)
        self._chk(self._L.oa_voxel_downsample(self._h, p, n, on_dev, pn, float(voxel), po, n, capi.fptr(out),
                                              capi.fptr(out_n) if out_n is not None else None, cnt.ctypes.data_as(i32p), capi.iptr(idx),
                                              C.byref(m), C.byref(rep)))
        rows = int(m.value)
        del keep, keep_n
        report = {"n_in": rep.n_in, "n_finite": rep.n_finite, "n_voxels": rep.n_voxels, "max_members": rep.max_members,
                  "dims": tuple(rep.dims), "origin": tuple(rep.origin), "total_ms": rep.total_ms}
        return {"xyz": out[:rows].copy(), "normals": out_n[:rows].copy() if out_n is not None else None, "count": cnt[:rows].copy(),
                "rep": idx[:rows].copy(), "report": report}

    def normal_space_sample(self, normals, m, grid=8, unoriented=False, seed=0):
        """Normal-space sampling (Rusinkiewicz & Levoy 2001) of ANY cloud's normals (no target, source or matrices needed; nothing a
        loop reads is touched): the normals are bucketed on a cube map of grid x grid cells per face and m points are drawn evenly
        across the buckets, so that the few normals of a small feature are all kept before a flat region gives its second point.
        normals: (n, 3) host array or torch device tensor, any length; zero and non-finite rows take no part.  unoriented: n and
        -n share a bucket (estimated normals).  seed: which members of a bucket come first (a hash of the index).  Returns a dict:
        idx int64 (min(m, eligible),) ascending -- a vlist --, bin int32 (n,) every point's bucket (-1: no part), report."""
        normals, m, grid, unoriented, seed = _sample_args(normals, m, grid, unoriented, seed)
        p, on_dev, keep, n = _device_ptr(normals)
        rep = capi.SampleReport()
        got = C.c_int64(0)
        cap = min(m, n)
        idx = np.empty(cap, np.int64)
        bins = np.empty(n, np.int32)
        self._chk(self._L.oa_normal_space_sample(self._h, p, n, on_dev, m, grid, unoriented, seed, cap, capi.iptr(idx),
                                                 bins.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(got), C.byref(rep)))
        del keep
        report = {name: getattr(rep, name) for name, _ in capi.SampleReport._fields_}
        return {"idx": idx[: int(got.value)].copy(), "bin": bins, "report": report}

    def stability(self, xyz, normals, idx=None):
        """Which rigid motions does a selection resist under the point-to-plane metric (Gelfand et al. 2003): the 6 x 6 matrix
        C = sum v v^T, v = [q x n ; n] over the points idx lists (None: all), q = (p - centroid) * scale with scale = 1 / mean
        |p - centroid|, and its eigen-decomposition.  xyz, normals: (n, 3) host arrays or torch device tensors (both on the same
        side); rows with a zero or non-finite normal or a non-finite coordinate take no part.  Returns a dict: n_used, centroid
        (3,), scale, C (6, 6), eigenvalues (6,) descending, eigenvectors (6, 6) -- COLUMN k belongs to eigenvalue k; its rows 0-2
        are a rotation about the centroid (in lengths times scale), its rows 3-5 a translation --, rank (eigenvalues above 1e-10
        times the largest), cond (largest over smallest eigenvalue), total_ms.
        How to read it: a small eigenvalue says that the selection does not resist this screw -- a loop over these points can slide
        along that motion, and noise decides that part of the pose.  rank < 6: some motion is not constrained at all (a plane
        3, a sphere 3, a cylinder 4); a large cond: one is constrained much more weakly than another."""
        xyz, normals, idx = _stability_args(xyz, normals, idx)
        p, on_dev, keep, n = _device_ptr(xyz)
        pn, _, keep_n, _ = _device_ptr(normals)
        rep = capi.StabilityReport()
        self._chk(self._L.oa_stability(self._h, p, pn, n, on_dev, capi.iptr(idx) if idx is not None else None,
                                       len(idx) if idx is not None else 0, C.byref(rep)))
        del keep, keep_n
        return {"n_used": int(rep.n_used), "centroid": np.array(rep.centroid, np.float64), "scale": float(rep.scale),
                "C": np.array(rep.C, np.float64).reshape(6, 6), "eigenvalues": np.array(rep.eigenvalues, np.float64),
                "eigenvectors": np.array(rep.eigenvectors, np.float64).reshape(6, 6), "rank": int(rep.rank), "cond": float(rep.cond),
                "total_ms": float(rep.total_ms)}

    def deviation(self, thresh=float("inf"), signed="auto", quantiles=(0.5, 0.9, 0.95, 0.99), bins=0, hist_range=None,
                  outputs=("signed_d", "closest", "idx", "feature")):
        """How good is the alignment at the current matrices, and where does it deviate: one correspondence search, then per
        selected source point (caller order) the arrays named in `outputs` -- signed_d float64 (negative inside a mesh target,
        or behind a point-cloud target's normals), dist float64 (the world-space pair distance the loop sees), closest float32
        (n, 3) base-local, idx int64 (-1: no correspondence), feature int8 (0 face, 1-3 edge ab / bc / ca, 4-6 vertex a / b / c;
        -1 in vertex mode) -- plus "report" (fitness = inliers with dist < thresh over all points, mean / rms / std / mean_signed
        over the inliers, max_dist and max_index over all valid points, "quantiles": {q: exact order statistic}, counts, which
        sign rule was used) and "hist" (bins + 2 int64 counts over hist_range of signed_d, under- and overflow first and last;
        None without bins).  signed: "auto" (when possible), True (required) or False.  Single-device contexts."""
        thresh, signed_mode, quantiles, bins, (lo, hi), outputs = _deviation_args(thresh, signed, quantiles, bins, hist_range, outputs)
        n = self.n_selected
        m = max(1, n)
        st = capi.DeviationSettings()
        st.thresh, st.signed_mode, st.n_quantiles, st.n_bins, st.hist_lo, st.hist_hi = thresh, signed_mode, len(quantiles), bins, lo, hi
        for k, q in enumerate(quantiles):
            st.quantiles[k] = q
        arr = {"signed_d": np.empty(m, np.float64) if "signed_d" in outputs else None,
               "dist": np.empty(m, np.float64) if "dist" in outputs else None,
               "closest": np.empty((m, 3), np.float32) if "closest" in outputs else None,
               "idx": np.empty(m, np.int64) if "idx" in outputs else None,
               "feature": np.empty(m, np.int8) if "feature" in outputs else None}
        hist = np.zeros(bins + 2, np.int64) if bins > 0 else None
        rep = capi.DeviationReport()
        self._chk(self._L.oa_deviation(
            self._h, C.byref(st),
            capi.dptr(arr["signed_d"]) if arr["signed_d"] is not None else None, capi.dptr(arr["dist"]) if arr["dist"] is not None else None,
            capi.fptr(arr["closest"]) if arr["closest"] is not None else None, capi.iptr(arr["idx"]) if arr["idx"] is not None else None,
            arr["feature"].ctypes.data_as(C.POINTER(C.c_int8)) if arr["feature"] is not None else None,
            capi.iptr(hist) if hist is not None else None, C.byref(rep)))
        report = {name: getattr(rep, name) for name, _ in capi.DeviationReport._fields_ if name not in ("reserved", "quantile_values", "n_quantiles")}
        report["quantiles"] = {q: float(rep.quantile_values[k]) for k, q in enumerate(quantiles)}
        report["thresh"] = thresh
        out = {name: a[:n] for name, a in arr.items() if a is not None}
        out["report"] = report
        out["hist"] = hist
        return out

    def mesh_pseudonormals(self):
        """Surface-mode targets: the angle-weighted pseudo-normals the signed distance uses, built on the device if they are not
        there yet: (vertex_n float32 (n_verts, 3), edge_n float32 (n_tris, 3, 3) -- one per triangle and local edge ab / bc / ca,
        the same bits on both sides of a shared edge).  Not normalised."""
        nt = int(self.stat("n_tris"))
        vn = np.empty((max(1, self.n_target), 3), np.float32)
        en = np.empty((max(1, nt), 3, 3), np.float32)
        self._chk(self._L.oa_get_mesh_pseudonormals(self._h, capi.fptr(vn), capi.fptr(en)))
        return vn[: self.n_target], en[:nt]

    # ---- split phase (one process per GPU)
    def run_begin(self, iters=50, thresh=0.5, target_d=0.01, use_target=True, with_scale=False, early_exit=True):
        st = self._settings(iters, thresh, target_d, use_target, with_scale, early_exit)
        self._chk(self._L.oa_run_begin(self._h, C.byref(st)))

    def iter_partial(self, sums_device_ptr: int):
        self._chk(self._L.oa_iter_partial(self._h, C.c_void_p(sums_device_ptr)))

    def iter_finish(self, sums_device_ptr: int):
        self._chk(self._L.oa_iter_finish(self._h, C.c_void_p(sums_device_ptr)))

    def run_end(self) -> RunResult:
        rep = capi.Report()
        rc = self._L.oa_run_end(self._h, C.byref(rep))
        if rc == capi.OA_E_TOO_FEW_PAIRS:
            raise ValueError(REF_VALUEERROR)
        self._chk(rc)
        return self._result(rep)


def device_count() -> int:
    return int(capi.load().oa_device_count())


def shard_bounds(n_selected: int, shard_index: int, shard_count: int):
    """[begin, end) of shard `shard_index` -- the same contiguous split oa_set_source applies."""
    per = -(-n_selected // shard_count) if shard_count > 0 else n_selected
    begin = min(n_selected, per * shard_index)
    return begin, min(n_selected, begin + per)
