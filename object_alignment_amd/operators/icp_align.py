"""Drop-in mirror of the reference's operators/icp_align.py (OBJECT_OT_icp_align).

`IcpAlign.run` is the Blender-free form of `execute` (operators/icp_align.py:82-161): the whole
`while n < iters and not converged` loop runs device-resident in liboa_icp.so (oa_run).
`OBJECT_OT_icp_align` keeps the operator surface (bl_idname / bl_label / bl_options / poll / execute) and
adapts duck-typed or real Blender objects to it.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ..engine import IcpEngine, RunResult
from ..functions.general import _coords_of, _matrix_to_np, _tris_of, default_engine, evaluated_base

try:                                              # inside Blender the operator registers as usual
    import bpy as _bpy                            # noqa: F401
    from bpy.types import Operator as _OperatorBase
except Exception:                                 # outside Blender it is a plain class
    _bpy = None
    _OperatorBase = object


@dataclass
class OutlierSettings:
    """What IcpSettings.clean_target / clean_source remove before anything else looks at a cloud (IcpEngine.target_outliers'
    arguments; checked here, before any engine opens).  method "statistical": a point stays when the mean distance to its k
    nearest neighbours is at most mean + std_ratio * std of that figure over the cloud; "radius": when at least min_neighbors other
    points lie within `radius`.  Lengths are in world units, like min_start."""
    method: str = "statistical"
    k: int = 16
    std_ratio: float = 2.0
    radius: float = 0.0
    min_neighbors: int = 8
    count_cap: int = 0

    def __post_init__(self):
        from ..engine import _outlier_args
        _outlier_args(**self.kwargs(1.0), name="OutlierSettings")

    def kwargs(self, scale):
        """The filter's arguments for a cloud whose local unit is `scale` world units (world_scale of its matrix)."""
        from ..engine import _real
        radius = self.radius / scale if _real(self.radius) else self.radius       # (anything else is for _outlier_args to refuse)
        return dict(method=self.method, k=self.k, std_ratio=self.std_ratio, radius=radius, min_neighbors=self.min_neighbors,
                    count_cap=self.count_cap)


@dataclass
class ClusterSettings:
    """What IcpSettings.segment_target / segment_source keep of a cloud: its DBSCAN clusters (IcpEngine.target_clusters' arguments;
    checked here, before any engine opens).  A point with at least min_points points within eps (itself included) is a core point,
    core points within eps of each other share a cluster, a point within eps of a core point joins its cluster, the rest is
    noise.  keep "largest": the largest cluster alone -- the scanned object without the table, the clamp or a second object --;
    "clustered": every cluster, the noise goes; "min_size": the clusters of at least min_size points.  eps is in world units, like
    min_start."""
    eps: float
    min_points: int = 8
    keep: str = "largest"
    min_size: int = 0

    def __post_init__(self):
        from ..engine import _cluster_args
        _cluster_args(**self.kwargs(1.0), name="ClusterSettings")

    def kwargs(self, scale):
        """The clustering's arguments for a cloud whose local unit is `scale` world units (world_scale of its matrix)."""
        from ..engine import _real
        eps = self.eps / scale if _real(self.eps) else self.eps               # (anything else is for _cluster_args to refuse)
        return dict(eps=eps, min_points=self.min_points, keep=self.keep, min_size=self.min_size)


@dataclass
class IcpSettings:
    """Names and defaults of the add-on preferences the loop reads (lib/preferences.py:31-72)."""
    icp_iterations: int = 50
    redraw_frequency: int = 10
    use_sample: bool = False          # never consulted by the reference either
    sample_fraction: float = 0.5
    min_start: float = 0.5
    target_d: float = 0.01
    use_target: bool = True
    take_m_with: bool = False
    align_meth: str = "0"             # '0' RIGID, '1' ROT_LOC_SCALE
    # not a preference of the reference: which GPUs the loop may use.  None = one GPU (or what the OA_DEVICES environment
    # variable lists); "all" / [0, 1, ...] = the source cloud is sharded over those GPUs inside the library
    devices: object = None
    # not a preference of the reference either (its citation.txt names both papers, its loop implements the first): what a
    # step minimises -- "point": the distance to the correspondence (Besl-McKay, the reference's loop); "plane": the distance
    # to the tangent plane at the correspondence (Chen-Medioni; rigid only, one GPU), which lets a surface slide along itself
    # "gicp": plane-to-plane (Generalized-ICP; rigid only, one GPU): every pair weighted by the normals of both sides -- needs
    # run(..., source_normals=...); gicp_epsilon is the small eigenvalue of its covariances, in [1e-6, 1]
    # "symmetric": the symmetric objective (Rusinkiewicz 2019; rigid only, one GPU): the plane metric's row with the mean of both
    # sides' normals, the rotation split between the two sides -- needs run(..., source_normals=...), no parameter
    metric: str = "point"
    gicp_epsilon: float = 1e-3
    # nor these: the weight of a pair in a step is a robust loss of its residual -- "none" (every pair weighs one, the
    # reference's loop), "huber", "tukey" or "cauchy" with the fixed scale robust_scale in world units, like min_start --
    # so that scan noise, a blob of wax or the rim of a partial overlap inside min_start pulls less than a good pair
    robust_loss: str = "none"
    robust_scale: float = 0.0
    # robust_quantile > 0: the loss's scale comes from each step's own residuals, c = max(robust_scale * q, robust_scale_min) with
    # q their robust_quantile-th order statistic, and robust_scale is a dimensionless multiplier (MAD_TUNING).  The floor is in
    # world units; None = target_d, the length the loop converges to
    robust_quantile: float = 0.0
    robust_scale_min: float | None = None
    # nor these: reciprocal=True keeps a pair of a step only if it is mutual -- the source point is also the nearest selected
    # source point of its own correspondence (reciprocal_ratio 1; up to 16: within that multiple of the nearest distance).  For
    # a source that reaches beyond the target (a whole model against a partial scan, two partial scans): the points outside the
    # overlap pair with the target's rim inside min_start, and those pairs are not mutual.  One GPU
    reciprocal: bool = False
    reciprocal_ratio: float = 1.0
    # nor these: Trimmed ICP -- trim > 0 keeps only that share of every step's pairs, the ones with the smallest residuals (the
    # overlap of the two clouds, if it is known); trim="auto" lets every step estimate the share itself (fractional ICP: the share
    # that minimises FRMSD with exponent trim_lambda, searched from trim_min up).  No scale in world units to choose, no tree over
    # the source, and displaced outliers go as well as the rim of an overlap.  0 = off.  One GPU
    trim: object = 0.0
    trim_min: float = 0.3
    trim_lambda: float = 2.0
    # nor these: reject_boundary=True drops a pair of a step whose correspondence lies on the target's boundary -- an edge of an
    # open mesh that one triangle owns, or a point on the rim of a cloud (the largest angular gap between its boundary_k nearest
    # neighbours, seen in the tangent plane, exceeds boundary_angle degrees; a cloud target then needs its normals).  The rim is a
    # property of the target alone, found once: the cheapest answer to a source that reaches beyond a partial scan.  One GPU
    reject_boundary: bool = False
    boundary_k: int = 16
    boundary_angle: float = 90.0
    # neighbours per vertex when run(..., target_normals="estimate") estimates a point-cloud target's normals on the device
    normal_k: int = 16
    # nor this: how an ESTIMATED normal field gets its signs, wherever run() estimates one (target_normals="estimate",
    # source_normals="estimate").  "away": every normal away from the cloud's centroid -- right for a star-shaped object only.
    # "consistent": the estimate is followed by IcpEngine.orient_target_normals (k = normal_k, seed away from the centroid, no
    # edge cap): signs handed along the minimum spanning forest of the neighbour graph (Hoppe et al. 1992), right for a torus, an
    # arch or a bent tube as well.  The normal-angle test, the sign of a cloud target's deviation and oriented normal-space
    # sampling read those signs
    normal_orient: str = "away"
    # nor this: > 0 thins the selection in SPACE before the loop -- one vertex per occupied cell of a grid of this edge (world
    # units, like min_start): the member nearest to the cell's mean (IcpEngine.voxel_downsample) -- so that a region the scanner
    # covered twice does not weigh twice; sample_fraction then applies to that list, as to any vlist.  0 = off: the selection is
    # thinned by index alone, as in the reference
    sample_voxel: float = 0.0
    # nor these: sample_normal_space > 0 keeps that many of the vertices the loop would have used, drawn evenly across the buckets
    # of their NORMALS (normal-space sampling, Rusinkiewicz & Levoy 2001; IcpEngine.normal_space_sample with sample_normal_grid
    # cells per edge of a cube face) -- on a mostly flat part the few vertices of a groove or a rim are all that stops sliding, and
    # a uniform sample holds next to none of them.  Needs run(..., source_normals=...).  0 = off
    sample_normal_space: int = 0
    sample_normal_grid: int = 8
    # nor these: an OutlierSettings removes the stray points of a raw scan -- flying pixels, dust, the scanner table -- before
    # anything else looks at the cloud.  clean_target: the point-cloud target is cleaned on the device right after its upload
    # (IcpEngine.target_outliers(apply=True)); normals are estimated, and every search runs, on what is left.  clean_source: the
    # vertices vlist selects go through object_alignment_amd.remove_outliers first, and the removed ones leave the selection
    # before sample_voxel thins it.  None = off.  One GPU
    clean_target: object = None
    clean_source: object = None
    # nor these: a ClusterSettings keeps the part of a raw scan that is the object -- what clean_* cannot remove because it is
    # dense: the scanner table, a clamp, a second object on the turntable.  segment_target: the point-cloud target is clustered on
    # the device right after clean_target (IcpEngine.target_clusters(apply=True)), before normals, features and the loop.
    # segment_source: the selection, after clean_source, goes through object_alignment_amd.cluster_dbscan.  None = off.  One GPU
    segment_target: object = None
    segment_source: object = None
    # nor these: a radius, in world units like min_start, that limits the neighbourhoods of per-vertex estimates on a raw cloud
    # (IcpEngine.set_neighbor_radius) -- the k nearest neighbours otherwise reach the other side of a thin wall, the next tooth or
    # across a hole.  normal_radius: the normals run() estimates, the target's and the source's (normal_k nearest within it; fewer
    # than three: the zero normal, which the metrics drop).  boundary_radius: the cloud criterion of reject_boundary.  Each is
    # carried to the cloud's own units by its matrix.  None = the k nearest however far, as before
    normal_radius: object = None
    boundary_radius: object = None

    def __post_init__(self):
        from ..engine import _radius_arg
        for name in ("normal_radius", "boundary_radius"):       # (checked again when a run reads them: neighbor_radii_of)
            if getattr(self, name) is not None:
                _radius_arg(getattr(self, name), "IcpSettings", name)


@dataclass
class DeviationSettings:
    """What IcpAlign.run(..., deviation=DeviationSettings()) measures at the final pose (IcpEngine.deviation's arguments; checked
    here, before any engine opens).  thresh None = the loop's min_start."""
    thresh: float | None = None
    signed: object = "auto"           # "auto" (when possible), True (required) or False
    quantiles: tuple = (0.5, 0.9, 0.95, 0.99)
    bins: int = 0
    hist_range: tuple | None = None
    outputs: tuple = ("signed_d", "closest", "idx", "feature")

    def __post_init__(self):
        from ..engine import _deviation_args
        _deviation_args(**self.kwargs(1.0), name="DeviationSettings")

    def kwargs(self, default_thresh):
        return dict(thresh=default_thresh if self.thresh is None else self.thresh, signed=self.signed, quantiles=self.quantiles,
                    bins=self.bins, hist_range=self.hist_range, outputs=self.outputs)


MAD_TUNING = {"huber": 1.345 * 1.4826, "tukey": 4.685 * 1.4826, "cauchy": 2.385 * 1.4826}
"""The usual constant-times-median choices of robust_scale for robust_quantile = 0.5: each loss's 95 %-efficiency tuning constant
times 1.4826, which carries the median of |residual| to the standard deviation of Gaussian noise (the MAD scale).
IcpSettings(robust_loss="tukey", robust_scale=MAD_TUNING["tukey"], robust_quantile=0.5) is the parameter-free setting."""


_prefs = IcpSettings()


def get_addon_preferences() -> IcpSettings:
    """Stand-in for functions/common/blender.py:48-55; returns the process-wide settings object."""
    return _prefs


def metric_of(settings) -> str:
    """IcpSettings.metric, or the `icp_metric` enum of the registered add-on preferences; "point" when neither is there."""
    return str(getattr(settings, "metric", None) or getattr(settings, "icp_metric", None) or "point")


def apply_metric(engine, settings) -> None:
    """Hand the settings' metric to the engine -- every time: the engine is shared and remembers the last one.  An engine
    without set_metric (a stand-in that only knows the reference's loop) is a point-metric engine."""
    metric = metric_of(settings)
    setter = getattr(engine, "set_metric", None)
    if setter is not None:
        setter(metric)
    elif metric != "point":
        raise RuntimeError("this engine has no %r metric" % metric)
    setter = getattr(engine, "set_gicp", None)
    if metric == "gicp" and setter is not None:
        setter(float(getattr(settings, "gicp_epsilon", 1e-3)))


def robust_of(settings):
    """(loss, scale) from IcpSettings.robust_loss / robust_scale, or the `icp_robust_loss` / `icp_robust_scale` preferences of
    the registered add-on; ("none", 0.0) when neither is there."""
    loss = getattr(settings, "robust_loss", None) or getattr(settings, "icp_robust_loss", None) or "none"
    scale = getattr(settings, "robust_scale", None)
    if scale is None:
        scale = getattr(settings, "icp_robust_scale", 0.0)
    return str(loss), float(scale or 0.0)


def robust_auto_of(settings):
    """(quantile, floor) from IcpSettings.robust_quantile / robust_scale_min, or the `icp_robust_quantile` /
    `icp_robust_scale_min` preferences of the registered add-on; (0.0, 0.0) -- off -- when neither is there.  A floor of None
    (or 0, the preference's "not set") is the settings' target_d."""
    quantile = getattr(settings, "robust_quantile", None)
    if quantile is None:
        quantile = getattr(settings, "icp_robust_quantile", 0.0)
    quantile = float(quantile or 0.0)
    if quantile == 0.0:
        return 0.0, 0.0
    floor = getattr(settings, "robust_scale_min", None)
    if floor is None:
        floor = getattr(settings, "icp_robust_scale_min", None)
    if not floor:
        floor = getattr(settings, "target_d", None)
    return quantile, float(floor or 0.0)


def apply_robust(engine, settings) -> None:
    """Hand the settings' robust loss and its estimated-scale setting to the engine -- every time, off included: the engine is
    shared and remembers the last ones.  An engine without set_robust counts as loss-none, one without set_robust_auto as a
    fixed-scale engine."""
    loss, scale = robust_of(settings)
    setter = getattr(engine, "set_robust", None)
    if setter is not None:
        setter(loss, scale)
    elif loss != "none":
        raise RuntimeError("this engine has no %r loss" % loss)
    quantile, floor = robust_auto_of(settings)
    setter = getattr(engine, "set_robust_auto", None)
    if setter is not None:
        setter(quantile, floor)
    elif quantile != 0.0:
        raise RuntimeError("this engine cannot estimate the robust scale")


def reciprocal_of(settings):
    """(on, ratio) from IcpSettings.reciprocal / reciprocal_ratio, or the `icp_reciprocal` / `icp_reciprocal_ratio` preferences
    of the registered add-on; (False, 1.0) when neither is there."""
    on = getattr(settings, "reciprocal", None)
    if on is None:
        on = getattr(settings, "icp_reciprocal", False)
    ratio = getattr(settings, "reciprocal_ratio", None)
    if ratio is None:
        ratio = getattr(settings, "icp_reciprocal_ratio", 1.0)
    return bool(on), float(ratio or 1.0)


def apply_reciprocal(engine, settings) -> None:
    """Hand the settings' reciprocal check to the engine -- every time, off included: the engine is shared and remembers the
    last setting.  An engine without set_reciprocal counts as one with the check off."""
    on, ratio = reciprocal_of(settings)
    setter = getattr(engine, "set_reciprocal", None)
    if setter is not None:
        setter(on, ratio)
    elif on:
        raise RuntimeError("this engine has no reciprocal check")


def trim_of(settings):
    """(fraction, fraction_min, lam) from IcpSettings.trim / trim_min / trim_lambda, or the `icp_trim` / `icp_trim_auto` /
    `icp_trim_min` preferences of the registered add-on; fraction is 0.0 (off), a share in (0, 1] or "auto".  (0.0, 0.3, 2.0)
    when neither is there."""
    frac = getattr(settings, "trim", None)
    if frac is None:
        frac = "auto" if getattr(settings, "icp_trim_auto", False) else getattr(settings, "icp_trim", 0.0)
    fmin = getattr(settings, "trim_min", None)
    if fmin is None:
        fmin = getattr(settings, "icp_trim_min", 0.3)
    lam = getattr(settings, "trim_lambda", None)
    if isinstance(frac, str):
        if frac != "auto":
            raise ValueError('trim must be a number or "auto", not %r' % (frac,))
    else:
        frac = float(frac or 0.0)
    return frac, float(fmin or 0.3), float(lam or 2.0)


def apply_trim(engine, settings) -> None:
    """Hand the settings' trim to the engine -- every time, off included: the engine is shared and remembers the last setting.
    An engine without set_trim counts as one with the trim off."""
    frac, fmin, lam = trim_of(settings)
    setter = getattr(engine, "set_trim", None)
    if setter is not None:
        setter(frac, fmin, lam)
    elif frac != 0.0:
        raise RuntimeError("this engine cannot trim its pairs")


def boundary_of(settings):
    """(on, k, angle_deg) from IcpSettings.reject_boundary / boundary_k / boundary_angle, or the `icp_reject_boundary` preference
    of the registered add-on; (False, 16, 90.0) when neither is there."""
    on = getattr(settings, "reject_boundary", None)
    if on is None:
        on = getattr(settings, "icp_reject_boundary", False)
    k = getattr(settings, "boundary_k", None)
    angle = getattr(settings, "boundary_angle", None)
    return bool(on), 16 if k is None else int(k), 90.0 if angle is None else float(angle)


def apply_boundary(engine, settings) -> None:
    """Hand the settings' boundary rejection to the engine -- every time, off included: the engine is shared and remembers the
    last setting.  An engine without set_reject_boundary counts as one with the setting off."""
    on, k, angle = boundary_of(settings)
    setter = getattr(engine, "set_reject_boundary", None)
    if setter is not None:
        setter(on, k, angle)
    elif on:
        raise RuntimeError("this engine cannot reject pairs on the target's boundary")


def sample_voxel_of(settings) -> float:
    """IcpSettings.sample_voxel, checked: 0.0 (off) or a finite length > 0 in world units."""
    v = getattr(settings, "sample_voxel", 0.0)
    if v is None:
        return 0.0
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (np.isfinite(v) and v >= 0):
        raise ValueError("IcpSettings.sample_voxel = %r (0 = off, or finite and > 0)" % (v,))
    return float(v)


def sample_normal_space_of(settings):
    """(points, grid) from IcpSettings.sample_normal_space / sample_normal_grid, checked: points 0 (off) or a whole number > 0,
    grid a whole number in 1 .. 32."""
    m = getattr(settings, "sample_normal_space", 0)
    g = getattr(settings, "sample_normal_grid", 8)
    m = 0 if m is None else m
    g = 8 if g is None else g
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or m < 0:
        raise ValueError("IcpSettings.sample_normal_space = %r (0 = off, or a whole number of points > 0)" % (m,))
    if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not 1 <= g <= 32:
        raise ValueError("IcpSettings.sample_normal_grid = %r (a whole number in 1 .. 32)" % (g,))
    return int(m), int(g)


def neighbor_radii_of(settings):
    """(normal_radius, boundary_radius) from IcpSettings, checked: each None (off) or a finite length > 0 in world units."""
    from ..engine import _radius_arg
    out = []
    for name in ("normal_radius", "boundary_radius"):
        v = getattr(settings, name, None)
        out.append(None if v is None else _radius_arg(v, "IcpSettings", name))
    return tuple(out)


def local_radius(radius, mx, what):
    """A world-space radius in the units of the cloud that mx places (None stays None), as ClusterSettings.kwargs carries eps."""
    return None if radius is None else radius / _local_scale(mx, what)


NORMAL_ORIENTS = ("away", "consistent")


def normal_orient_of(settings) -> str:
    """IcpSettings.normal_orient, checked: "away" or "consistent"."""
    v = getattr(settings, "normal_orient", "away")
    if not isinstance(v, str) or v not in NORMAL_ORIENTS:
        raise ValueError("IcpSettings.normal_orient = %r (use 'away' or 'consistent')" % (v,))
    return v


def estimate_consistent_normals(xyz, k, device=0, radius=None):
    """PCA normals of a cloud with one consistent sign: the estimate (neighbours within `radius` of xyz's own units, None: the k
    nearest), then IcpEngine.orient_target_normals on it (seed away from the centroid), in a context of its own."""
    from ..engine import IcpEngine
    with IcpEngine(int(device)) as eng:
        eng.set_target(xyz)
        eng.estimate_target_normals(k=k, orient="none", install=True, radius=radius)
        return eng.orient_target_normals(k=k, max_dist=0.0, seed="away", install=False)[0]


def world_scale(mx) -> float:
    """cbrt(|det(mx[:3, :3])|): what carries a world-space length to the object's local space."""
    return float(np.cbrt(abs(np.linalg.det(np.asarray(mx, np.float64).reshape(4, 4)[:3, :3]))))


def voxel_vlist(engine, source_xyz, vlist, mx_align, sample_voxel):
    """One vertex per occupied voxel of edge sample_voxel (world units) among the vertices vlist selects (None: all): the
    representatives, as indices into source_xyz, ascending -- a vlist.  Vertices with a non-finite coordinate are in no voxel."""
    s = world_scale(mx_align)
    if not (np.isfinite(s) and s > 0):
        raise ValueError("sample_voxel needs an invertible matrix_world (scale %r)" % (s,))
    sel = None
    pts = source_xyz
    if vlist is not None:
        sel = np.ascontiguousarray(vlist, dtype=np.int64)
        if hasattr(pts, "is_cuda"):
            pts = pts.detach().cpu().numpy()
        pts = np.asarray(pts, np.float32).reshape(-1, 3)[sel]
    if getattr(engine, "multi", False):                        # (a multi-device context has no call of its own for it)
        from .. import voxel_downsample
        down = voxel_downsample(pts, sample_voxel / s, device=engine.device)
    else:
        call = getattr(engine, "voxel_downsample", None)
        if call is None:
            raise RuntimeError("this engine has no voxel downsample")
        down = call(pts, sample_voxel / s)
    rep = down["rep"]
    return np.sort(sel[rep] if sel is not None else rep)


def _host_rows(a):
    if hasattr(a, "is_cuda"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.float32).reshape(-1, 3)


def clean_of(settings):
    """(clean_target, clean_source) from IcpSettings: each an OutlierSettings or None."""
    out = []
    for name in ("clean_target", "clean_source"):
        v = getattr(settings, name, None)
        if v is not None and not isinstance(v, OutlierSettings):
            raise TypeError("IcpSettings.%s = %r (an OutlierSettings, or None)" % (name, v))
        out.append(v)
    return tuple(out)


def segment_of(settings):
    """(segment_target, segment_source) from IcpSettings: each a ClusterSettings or None."""
    out = []
    for name in ("segment_target", "segment_source"):
        v = getattr(settings, name, None)
        if v is not None and not isinstance(v, ClusterSettings):
            raise TypeError("IcpSettings.%s = %r (a ClusterSettings, or None)" % (name, v))
        out.append(v)
    return tuple(out)


def _local_scale(mx, what):
    s = world_scale(mx)
    if not (np.isfinite(s) and s > 0):
        raise ValueError("%s needs an invertible matrix_world (scale %r)" % (what, s))
    return s


def clean_resident_target(engine, clean, mx_base):
    """Remove the stray points of the engine's resident point-cloud target (IcpEngine.target_outliers(apply=True), lengths carried
    from world units to the target's own by mx_base): {"index": the kept vertices in the caller's numbering, "keep", "report"}."""
    call = getattr(engine, "target_outliers", None)
    if call is None:
        raise RuntimeError("this engine has no outlier removal")
    out = call(apply=True, **clean.kwargs(_local_scale(mx_base, "clean_target")))
    return {"index": out["index"], "keep": out["keep"], "report": out["report"]}


def clean_selection(engine, clean, source_xyz, vlist, mx_align):
    """The vertices vlist selects (None: all) without their stray points (object_alignment_amd.remove_outliers in a context of its
    own, lengths carried to the source's own units by mx_align): {"vlist": what is left, as indices into source_xyz in vlist's
    order, "index": the kept positions within the selection, "keep", "report"}."""
    from .. import remove_outliers
    scale = _local_scale(mx_align, "clean_source")
    pts = _host_rows(source_xyz)
    sel = None
    if vlist is not None:
        sel = np.ascontiguousarray(vlist, dtype=np.int64)
        pts = pts[sel]
    out = remove_outliers(pts, device=getattr(engine, "device", 0), **clean.kwargs(scale))
    index = out["index"].astype(np.int64)
    return {"vlist": sel[index] if sel is not None else index, "index": out["index"], "keep": out["keep"], "report": out["report"]}


def segment_resident_target(engine, seg, mx_base):
    """Keep the clusters `seg` names of the engine's resident point-cloud target (IcpEngine.target_clusters(apply=True), eps carried
    from world units to the target's own by mx_base): {"index": the kept vertices in the resident target's numbering, "label",
    "sizes", "keep", "report"}."""
    call = getattr(engine, "target_clusters", None)
    if call is None:
        raise RuntimeError("this engine has no clustering")
    out = call(apply=True, **seg.kwargs(_local_scale(mx_base, "segment_target")))
    return {name: out[name] for name in ("index", "label", "sizes", "keep", "report")}


def segment_selection(engine, seg, source_xyz, vlist, mx_align):
    """The vertices vlist selects (None: all) that lie in the clusters `seg` names (object_alignment_amd.cluster_dbscan in a context of
    its own, eps carried to the source's own units by mx_align): {"vlist": what is left, as indices into source_xyz in vlist's
    order, "index": the kept positions within the selection, "label", "sizes", "keep", "report"}."""
    from .. import cluster_dbscan
    scale = _local_scale(mx_align, "segment_source")
    pts = _host_rows(source_xyz)
    sel = None
    if vlist is not None:
        sel = np.ascontiguousarray(vlist, dtype=np.int64)
        pts = pts[sel]
    out = cluster_dbscan(pts, device=getattr(engine, "device", 0), **seg.kwargs(scale))
    index = out["index"].astype(np.int64)
    res = {name: out[name] for name in ("index", "label", "sizes", "keep", "report")}
    res["vlist"] = sel[index] if sel is not None else index
    return res


def normal_space_vlist(engine, source_xyz, source_normals, vlist, stride, m, grid, unoriented):
    """m of the vertices a loop over (vlist, stride) would use -- vlist[0::stride], None: every vertex --, drawn evenly across
    the buckets of their normals (IcpEngine.normal_space_sample): {"idx": their indices into source_xyz, in the candidates' order
    -- a vlist for stride 1 --, "report": the sampling report, "stability": IcpEngine.stability of the picked set}."""
    normals = _host_rows(source_normals)
    n = len(normals)
    cand = np.arange(n, dtype=np.int64) if vlist is None else np.ascontiguousarray(vlist, dtype=np.int64)
    cand = cand[:: max(1, int(stride))]
    if getattr(engine, "multi", False):                        # (a multi-device context has no calls of its own for these)
        from .. import normal_space_sample, stability
        dev = {"device": engine.device}
    else:
        normal_space_sample, stability = getattr(engine, "normal_space_sample", None), getattr(engine, "stability", None)
        if normal_space_sample is None or stability is None:
            raise RuntimeError("this engine has no normal-space sampling")
        dev = {}
    drawn = normal_space_sample(normals if vlist is None and max(1, int(stride)) == 1 else normals[cand], m, grid=grid,
                                unoriented=unoriented, **dev)
    picked = cand[drawn["idx"]]
    return {"idx": picked, "report": drawn["report"], "stability": stability(_host_rows(source_xyz), normals, idx=picked, **dev)}


def build_vlist(align_obj):
    """Vertex indices the operator aligns with, from the object's `icp_include` / `icp_exclude` vertex groups
    (semantics of operators/icp_align.py:56-80): an include group wins and keeps memberships heavier than 0.9;
    otherwise an exclude group drops every vertex whose membership weighs 0.1 or more; no group = every vertex."""
    mesh = getattr(align_obj, "data", None)
    if mesh is None:
        return list(range(len(_coords_of(align_obj))))
    group_index = {g.name: g.index for g in (getattr(align_obj, "vertex_groups", None) or ())}

    def weights_in(vertex, gi):
        return [m.weight for m in vertex.groups if m.group == gi]

    if "icp_include" in group_index:
        gi = group_index["icp_include"]
        # one entry per qualifying membership, exactly as the reference appends inside its inner loop
        return [v.index for v in mesh.vertices for w in weights_in(v, gi) if w > 0.9]
    if "icp_exclude" in group_index:
        gi = group_index["icp_exclude"]
        keep = []
        for v in mesh.vertices:
            ws = weights_in(v, gi)
            if not ws:
                keep.append(v.index)
            else:
                keep.extend(v.index for w in ws if w < 0.1)
        return keep
    return [v.index for v in mesh.vertices]


def vlist_for_engine(align_obj):
    """build_vlist() for the engine: None when the object has neither an `icp_include` nor an `icp_exclude` group --
    the engine then takes every vertex itself, and a million-element Python list is neither built nor converted."""
    names = {g.name for g in (getattr(align_obj, "vertex_groups", None) or ())}
    if "icp_include" in names or "icp_exclude" in names:
        return build_vlist(align_obj)
    return None


def vlist_from_weights(n_verts, include=None, exclude=None):
    """Array form of the same mask: include / exclude are None or iterables of (vertex_index, weight)."""
    if include is not None:
        return [int(v) for v, w in sorted(include, key=lambda t: t[0]) if np.float32(w) > 0.9]
    if exclude is not None:
        member = {int(v): np.float32(w) for v, w in exclude}
        return [v for v in range(n_verts) if v not in member or member[v] < 0.1]
    return list(range(n_verts))


class IcpAlign:
    """The ICP loop of OBJECT_OT_icp_align.execute without Blender."""

    def __init__(self, settings: IcpSettings | None = None, engine: IcpEngine | None = None):
        self.settings = settings if settings is not None else get_addon_preferences()
        self._engine = engine

    @property
    def engine(self):
        """The engine the loop runs on: the one given, else the process-wide default one, opened on first use."""
        if self._engine is None:
            self._engine = default_engine(devices=getattr(self.settings, "devices", None))
        return self._engine

    @engine.setter
    def engine(self, engine):
        self._engine = engine

    def run(self, source_xyz, target_xyz, mx_align, mx_base, vlist=None, early_exit=True,
            target_tris=None, target_normals=None, source_weights=None, coarse=None, source_normals=None, deviation=None) -> RunResult:
        """target_tris: (n, 3) triangles of the base mesh -> closest point on the surface (the reference's BVH
        semantics); None -> nearest target vertex (point-cloud targets, BASELINE's configurations).
        target_normals: one normal per target vertex -- what settings.metric == "plane" needs of a point-cloud target -- or
        "estimate": PCA normals from every target vertex's settings.normal_k nearest neighbours, computed on the device after
        the upload and oriented away from the target's centroid -- or, with settings.normal_orient == "consistent", along the
        minimum spanning forest of the neighbour graph (point-cloud targets only: a mesh has its triangles').
        source_weights: one weight per vertex of source_xyz (finite, >= 0) -- "trust this region less"; None = all one.
        source_normals: one align-local normal per vertex of source_xyz -- what settings.metric == "gicp" / "symmetric" needs -- or "estimate":
        object_alignment_amd.estimate_normals(source_xyz, k=settings.normal_k), in a context of its own (those metrics do not
        look at the normals' signs, so they are left unoriented; settings.normal_orient == "consistent" gives them one sign).
        coarse: a CoarseSettings (operators/coarse_align.py) -- the coarse global stage runs on the same engine in front of the
        loop, which then starts from the pose it found (self.last_coarse holds its report); None: the loop alone.
        settings.sample_voxel > 0: the vertices vlist selects are first thinned to one representative per voxel of that edge
        (voxel_vlist); sample_fraction then applies to that list.
        settings.sample_normal_space > 0: of the vertices the loop would then use -- vlist, thinned by sample_voxel, every
        round(1 / sample_fraction)-th of that -- that many are kept, drawn evenly across the buckets of their normals
        (normal_space_vlist; n and -n share a bucket when the normals were estimated).  Needs source_normals (ValueError
        otherwise).  self.last_sampling holds the picked indices, the sampling report and the stability report of the picked set;
        None while the setting is off.
        settings.clean_target / clean_source: an OutlierSettings each -- the point-cloud target loses its stray points right after
        the upload (a target_normals array is gathered to what is left, an estimate sees only that; ValueError with target_tris),
        the selection loses its own before sample_voxel.  self.last_cleaning = {"target": ..., "source": ...} holds the index maps
        and reports (None for a side that was not cleaned); None while both settings are off.  An attached deviation report's idx
        speaks of the caller's target vertices.
        settings.segment_target / segment_source: a ClusterSettings each -- right after clean_target the point-cloud target keeps
        the clusters the setting names (ValueError with target_tris), the selection its own right after clean_source.
        self.last_segmentation = {"target": ..., "source": ...} holds, per side, "index" -- the kept vertices in the CALLER's
        numbering (the target's vertices; positions within the selection), composed with a preceding clean step --, "label" and
        "sizes" over the cloud the clustering saw, and the report; None while both settings are off.
        deviation: a DeviationSettings -- after the loop the deviation report and its arrays are taken at the final pose on the same
        engine (over the points the loop used) and attached as RunResult.deviation; None: nothing else changes.
        settings.normal_radius / boundary_radius: world-space lengths that limit the neighbourhoods of the estimated normals (the
        target's by mx_base's scale, the source's by mx_align's) and of the cloud criterion behind reject_boundary (mx_base's)."""
        s = self.settings
        normal_radius, boundary_radius = neighbor_radii_of(s)
        estimate = isinstance(target_normals, str)
        if estimate and target_normals != "estimate":
            raise ValueError("target_normals %r (an array of normals, or 'estimate')" % (target_normals,))
        if estimate and target_tris is not None:
            raise ValueError("target_normals='estimate' is for point-cloud targets: a mesh (target_tris) uses its triangles' normals")
        if isinstance(source_normals, str) and source_normals != "estimate":
            raise ValueError("source_normals %r (an array of normals, or 'estimate')" % (source_normals,))
        if deviation is not None and not isinstance(deviation, DeviationSettings):
            raise TypeError("deviation %r (a DeviationSettings, or None)" % (deviation,))
        sample_voxel = sample_voxel_of(s)
        sample_normals, sample_grid = sample_normal_space_of(s)
        consistent = normal_orient_of(s) == "consistent"
        if sample_normals > 0 and source_normals is None:
            raise ValueError("IcpSettings.sample_normal_space needs source_normals (an array of normals, or 'estimate')")
        clean_target, clean_source = clean_of(s)
        if clean_target is not None and target_tris is not None:
            raise ValueError("IcpSettings.clean_target is for point-cloud targets: a mesh (target_tris) has no stray vertices to remove")
        segment_target, segment_source = segment_of(s)
        if segment_target is not None and target_tris is not None:
            raise ValueError("IcpSettings.segment_target is for point-cloud targets: a mesh (target_tris) is one connected surface already")
        thresh = s.min_start                                   # :83
        factor = round(1 / s.sample_fraction)                  # :89  (ZeroDivisionError at 0, as the reference)
        if not thresh > 0:
            # make_pairs returns None and `(A, B, d_stats) = None` raises   (:101, general.py:277)
            raise TypeError("cannot unpack non-iterable NoneType object")
        eng = self.engine
        normal_r_tgt = local_radius(normal_radius, mx_base, "normal_radius") if estimate else None
        boundary_r = local_radius(boundary_radius, mx_base, "boundary_radius") if (boundary_of(s)[0] and target_tris is None) else None
        cleaning = {"target": None, "source": None}
        self.last_cleaning = cleaning if (clean_target is not None or clean_source is not None) else None
        segmentation = {"target": None, "source": None}
        self.last_segmentation = segmentation if (segment_target is not None or segment_source is not None) else None
        target_kept = None                                     # the resident target's vertices in the caller's numbering, once some left
        if target_tris is not None:
            eng.set_target_mesh(target_xyz, target_tris)
        else:
            eng.set_target(target_xyz)
            if clean_target is not None:
                cleaning["target"] = clean_resident_target(eng, clean_target, mx_base)
                target_kept = cleaning["target"]["index"]
            if segment_target is not None:
                segmentation["target"] = segment_resident_target(eng, segment_target, mx_base)
                if target_kept is not None:
                    segmentation["target"]["index"] = target_kept[segmentation["target"]["index"]]
                target_kept = segmentation["target"]["index"]
            if target_kept is not None and target_normals is not None and not estimate:
                target_normals = np.asarray(target_normals).reshape(-1, 3)[target_kept]
            if estimate:
                if normal_r_tgt is None:
                    eng.estimate_target_normals(k=int(getattr(s, "normal_k", 16)), orient="away", install=True)
                else:
                    eng.estimate_target_normals(k=int(getattr(s, "normal_k", 16)), orient="away", install=True, radius=normal_r_tgt)
                if consistent:
                    eng.orient_target_normals(k=int(getattr(s, "normal_k", 16)), max_dist=0.0, seed="away", install=True)
            elif target_normals is not None:
                eng.set_target_normals(target_normals)
        apply_metric(eng, s)
        apply_robust(eng, s)
        apply_reciprocal(eng, s)
        apply_trim(eng, s)
        apply_boundary(eng, s)
        if clean_source is not None:
            cleaning["source"] = clean_selection(eng, clean_source, source_xyz, vlist, mx_align)
            vlist = cleaning["source"]["vlist"]
        if segment_source is not None:
            segmentation["source"] = segment_selection(eng, segment_source, source_xyz, vlist, mx_align)
            vlist = segmentation["source"]["vlist"]
            if cleaning["source"] is not None:
                segmentation["source"]["index"] = cleaning["source"]["index"][segmentation["source"]["index"]]
        if sample_voxel > 0.0:
            vlist = voxel_vlist(eng, source_xyz, vlist, mx_align, sample_voxel)
        estimate_source = isinstance(source_normals, str)

        def estimated_source_normals():
            kw = {} if normal_radius is None else {"radius": local_radius(normal_radius, mx_align, "normal_radius")}
            if consistent:
                return estimate_consistent_normals(source_xyz, int(getattr(s, "normal_k", 16)), **kw)
            from .. import estimate_normals
            return estimate_normals(source_xyz, k=int(getattr(s, "normal_k", 16)), **kw)[0]

        # the source's normals are estimated ONCE: in front of the upload when the sample needs them, else behind it, where the
        # estimate has always stood (so that a run without the sample makes its calls in the order it always did)
        self.last_sampling = None
        if sample_normals > 0:
            if estimate_source:
                source_normals = estimated_source_normals()
            self.last_sampling = normal_space_vlist(eng, source_xyz, source_normals, vlist, factor, sample_normals, sample_grid, estimate_source)
            vlist, factor = self.last_sampling["idx"], 1
        eng.set_source(source_xyz, vlist=vlist, stride=factor)
        if source_weights is not None:
            eng.set_source_weights(source_weights)
        if estimate_source and sample_normals == 0:
            source_normals = estimated_source_normals()
        if source_normals is not None:
            eng.set_source_normals(source_normals)
        eng.set_matrices(mx_align, mx_base)
        self.last_coarse = None
        if coarse is not None:
            from .coarse_align import coarse_stage
            if target_kept is not None:                        # (the coarse stage thins the target it is given: the resident one)
                target_xyz = _host_rows(target_xyz)[target_kept]
            self.last_coarse = coarse_stage(eng, coarse, target_xyz, mx_base, source_xyz=source_xyz)
        if boundary_r is None:
            res = eng.run(iters=s.icp_iterations, thresh=thresh, target_d=s.target_d, use_target=s.use_target,
                          with_scale=(s.align_meth == "1"), early_exit=early_exit)
        else:
            # the loop builds the target's mask when it starts: the radius is the engine's setting for that long, and the mask
            # stays keyed by it (target_boundary(radius=...) afterwards returns the mask the loop used)
            prev = eng.neighbor_radius
            eng.set_neighbor_radius(boundary_r)
            try:
                res = eng.run(iters=s.icp_iterations, thresh=thresh, target_d=s.target_d, use_target=s.use_target,
                              with_scale=(s.align_meth == "1"), early_exit=early_exit)
            finally:
                eng.set_neighbor_radius(prev)
        if deviation is not None:
            res.deviation = eng.deviation(**deviation.kwargs(thresh))
            if target_kept is not None and res.deviation.get("idx") is not None:
                # the report speaks of the caller's vertices, not of the cleaned target's
                idx, kept = res.deviation["idx"], target_kept.astype(np.int64)
                res.deviation["idx"] = np.where(idx >= 0, kept[np.maximum(idx, 0)], -1)
        return res


def report_lines(res: RunResult, settings, seconds=None):
    """What the reference's execute prints when its loop ends (operators/icp_align.py:145-160), from the device's report: the
    convergence line or 'Maxed out iterations', then the last translation, the last d_stats and the mean of the 5-slot
    rotation ring -- same wording, same %f formats."""
    lines = []
    if settings.use_target and res.iters_done > 0:
        lines.append('Converged in %s iterations' % str(res.iters_done) if res.converged else 'Maxed out iterations')   # :145 / :154
        lines.append('Final Translation: %f ' % res.last_translation)                                                    # :146 / :155
        lines.append('Final Avg Dist: %f' % res.mean_dist)                                                               # :147 / :156
        lines.append('Final St Dev %f' % res.std_dist)                                                                   # :148 / :157
        lines.append('Avg last 5 rotation angle: %f' % res.mean_rot_angle)                                               # :149 / :158
    if seconds is not None:
        lines.append('Aligned obj in %f sec' % seconds)                                                                  # :160
    return lines


def _assign_matrix(obj, new_np):
    old = obj.matrix_world
    if isinstance(old, np.ndarray):
        obj.matrix_world = np.array(new_np, dtype=np.float32)
        return
    try:
        obj.matrix_world = type(old)([[float(x) for x in row] for row in new_np])
    except Exception:
        obj.matrix_world = np.array(new_np, dtype=np.float32)


def execute_alignment(op, context):
    """The body of `execute` of BOTH ICP operators: the reference's OBJECT_OT_icp_align.execute (operators/icp_align.py:47-161)
    and OBJECT_OT_icp_align_feedback.execute (operators/icp_align_feedback.py:130-235) are the same loop -- the second lacks
    the per-iteration timing prints, nothing else -- so both classes run this."""
    settings = get_addon_preferences()
    align_obj = context.object
    base_obj = next(o for o in context.selected_objects if o != align_obj)
    try:
        align_obj.rotation_mode = 'QUATERNION'
    except Exception:
        pass
    import time
    start = time.time()                                     # :51
    vlist = vlist_for_engine(align_obj)
    base_geo = evaluated_base(base_obj, context)            # BVHTree.FromObject(base_obj, depsgraph)  (:52-53)
    failure = None
    try:
        res = IcpAlign(settings).run(_coords_of(align_obj), _coords_of(base_geo),
                                     _matrix_to_np(align_obj.matrix_world), _matrix_to_np(base_obj.matrix_world),
                                     vlist=vlist, target_tris=_tris_of(base_geo))
    except ValueError as exc:
        # fewer than 3 pairs in iteration n: the reference has already applied iterations 0..n-1 to align_obj and
        # the m_* objects when affine_matrix_from_points raises (:109 after :121-127 of the earlier passes)
        res = getattr(exc, "partial", None)
        if res is None:
            raise
        failure = exc
    _assign_matrix(align_obj, res.matrix_world)
    if settings.take_m_with:                                # :123-127, replayed in iteration order
        from .. import _hostmath
        scene = getattr(context, "scene", None) or getattr(getattr(_bpy, "context", None), "scene", None)
        for obj in (scene.objects if scene is not None else []):
            if obj.name[:2] == "m_":
                m = _matrix_to_np(obj.matrix_world)
                for new_mat in res.step_new:
                    m = _hostmath.mat4_mul(m, new_mat)
                _assign_matrix(obj, m)
                if hasattr(obj, "update_tag"):
                    obj.update_tag()
    if hasattr(align_obj, "update_tag"):
        align_obj.update_tag()
    if hasattr(context, "view_layer") and hasattr(context.view_layer, "update"):
        context.view_layer.update()
    op.last_result = res
    # the reference prints its summary (:145-160); here it also goes to Blender's info area
    op.last_report = report_lines(res, settings, time.time() - start)
    for line in op.last_report:
        print(line)
        if hasattr(op, "report"):
            try:
                op.report({'INFO'}, line)
            except Exception:
                pass
    if failure is not None:
        raise failure
    return {'FINISHED'}


class OBJECT_OT_icp_align(_OperatorBase):
    """Iterative-closest-point alignment of the active object onto the other selected object"""
    bl_idname = "object.align_icp"
    bl_label = "ICP Align"
    bl_options = {'REGISTER', 'UNDO'}

    @classmethod
    def poll(cls, context):
        # exactly two selected objects, the active one a mesh (operators/icp_align.py:41-45)
        return len(context.selected_objects) == 2 and context.object.type == 'MESH'

    def execute(self, context):
        return execute_alignment(self, context)
