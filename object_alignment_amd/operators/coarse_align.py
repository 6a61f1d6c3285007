"""Coarse global alignment in front of the ICP loop (no counterpart in the reference, whose remedy for a bad start is picking
landmarks by hand, operators/align_pick_points.py).

`CoarseAlign.run` is "align these two scans" without landmarks: a few hundred candidate poses -- the source turned about its
centroid by a super-Fibonacci set of rotations, centroid on centroid -- are scored on the GPU in one launch by the truncated mean
distance of a sample to the target, the best few get a short point loop, and the cheapest becomes matrix_world
(oa_coarse_align).  `IcpAlign.run(..., coarse=CoarseSettings())` runs it on the same engine in front of the usual loop.

A source that is a PART of the target (one tooth against an arch, two passes that overlap by half) has its centroid far from the
target's: no rotation about it is near the answer.  `CoarseSettings(method="features")` takes the candidates from matched local
shape descriptors instead (FPFH of both clouds, mutual nearest rows, rigid motions of triples of matched points:
oa_target_fpfh, oa_feature_candidates) and hands them to the same scoring and refinement (oa_coarse_align_poses);
`method="both"` scores the two lists together.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ..functions.general import default_engine

METHODS = ("rotations", "features", "both")
THRESH_FRACTION = 0.1       # thresh=None: this part of the target's world-space bounding-box diagonal


@dataclass
class CoarseSettings:
    n_rot: int = 256                # rotation candidates
    n_refine: int = 8               # best candidates that get a short loop
    refine_iters: int = 10          # iterations of that loop
    stride: int = 4                 # every stride-th point of the selection is scored and refined
    thresh: float | None = None     # truncation / pair distance, world units; None = THRESH_FRACTION x the target's diagonal
    method: str = "rotations"       # where the candidates come from: "rotations", "features" (vertex-mode targets) or "both"
    feature_k: int = 16             # neighbours per FPFH descriptor
    normal_k: int = 16              # neighbours per estimated normal (the source's; the target's when none are installed)
    n_hyp: int = 4096               # triples of matched points
    edge_tol: float = 0.9           # a triple's edge lengths must agree within [edge_tol, 1 / edge_tol]
    ratio: float = 0.9              # nearest / second nearest descriptor distance (not squared) a match may have
    mutual: bool = True             # a match must be the nearest row in both directions
    seed: int = 0                   # of the hashed draw of the triples
    # method "features" / "both": None = descriptors of every target and source vertex; a length in world units = descriptors
    # of the two clouds' voxel downsamples of that edge (the coarse stage needs no more, and the matching is quadratic)
    voxel: float | None = None
    # method "features" / "both": a length in world units that limits the neighbourhoods of the descriptors, and of the normals
    # estimated for them, on both clouds (IcpEngine.set_neighbor_radius; each cloud's matrix carries it to its own units); None
    # = the feature_k / normal_k nearest however far
    feature_radius: object = None

    def __post_init__(self):
        if self.feature_radius is not None:
            from ..engine import _radius_arg
            _radius_arg(self.feature_radius, "CoarseSettings", "feature_radius")
        if self.method not in METHODS:
            raise ValueError("CoarseSettings.method = %r (one of %s)" % (self.method, ", ".join(repr(m) for m in METHODS)))
        for name, lo, hi in (("feature_k", 4, 64), ("normal_k", 3, 64), ("n_hyp", 1, 65535), ("seed", 0, 0xFFFFFFFF)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError("CoarseSettings.%s = %r (an integer in %d .. %d)" % (name, v, lo, hi))
        if not (isinstance(self.edge_tol, (int, float)) and 0.0 < self.edge_tol <= 1.0):
            raise ValueError("CoarseSettings.edge_tol = %r (in (0, 1])" % (self.edge_tol,))
        if not (isinstance(self.ratio, (int, float)) and np.isfinite(self.ratio) and self.ratio > 0.0):
            raise ValueError("CoarseSettings.ratio = %r (finite and > 0)" % (self.ratio,))
        if not isinstance(self.mutual, (bool, np.bool_)):
            raise ValueError("CoarseSettings.mutual = %r (True or False)" % (self.mutual,))
        for name, lo, hi in (("n_rot", 1, 65536), ("n_refine", 1, 4096), ("refine_iters", 0, 10000), ("stride", 1, 1 << 30)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError("CoarseSettings.%s = %r (an integer in %d .. %d)" % (name, v, lo, hi))
        if self.thresh is not None and not (np.isfinite(self.thresh) and self.thresh > 0):
            raise ValueError("CoarseSettings.thresh = %r (finite and > 0, or None)" % (self.thresh,))
        if self.voxel is not None and not (isinstance(self.voxel, (int, float, np.integer, np.floating)) and not isinstance(self.voxel, bool)
                                           and np.isfinite(self.voxel) and self.voxel > 0):
            raise ValueError("CoarseSettings.voxel = %r (finite and > 0, or None)" % (self.voxel,))


def default_thresh(target_xyz, mx_base) -> float:
    """THRESH_FRACTION x the diagonal of the target's axis-aligned bounding box in world space."""
    t = np.asarray(target_xyz, np.float64).reshape(-1, 3)
    m = np.asarray(mx_base, np.float64).reshape(4, 4)
    w = t @ m[:3, :3].T + m[:3, 3]
    w = w[np.all(np.isfinite(w), axis=1)]
    if len(w) == 0:
        raise ValueError("the target has no finite vertex")
    return THRESH_FRACTION * float(np.linalg.norm(w.max(axis=0) - w.min(axis=0)))


def _feature_radii(settings, mx_align, mx_base):
    """({} or {"radius": r}) for the target's calls and for the source's: settings.feature_radius in each cloud's own units."""
    r = getattr(settings, "feature_radius", None)
    if r is None:
        return {}, {}
    from ..engine import _radius_arg
    from .icp_align import local_radius
    r = _radius_arg(r, "CoarseSettings", "feature_radius")
    return ({"radius": local_radius(r, mx_base, "feature_radius")}, {"radius": local_radius(r, mx_align, "feature_radius")})


def feature_poses(engine, settings: CoarseSettings, source_xyz, mx_base=None) -> tuple:
    """Candidate poses from matched FPFH descriptors on an engine whose vertex-mode target, source and matrices are set:
    ((n, 4, 4) float32, report dict).  Installs estimated target normals (away from the centroid) when the target has none.
    mx_base: the target's matrix, what carries settings.feature_radius to the target's units (needed with that setting)."""
    from .. import fpfh
    if getattr(settings, "feature_radius", None) is not None and mx_base is None:
        raise ValueError("CoarseSettings.feature_radius needs mx_base")
    kw_tgt, kw_src = {}, {}
    if getattr(settings, "feature_radius", None) is not None:
        kw_tgt, kw_src = _feature_radii(settings, engine.matrix_world(), mx_base)
    rep = {"estimated_target_normals": False}
    if engine.stat("target_normals") == 0.0:
        engine.estimate_target_normals(k=min(settings.normal_k, engine.n_target), orient="away", install=True, **kw_tgt)
        rep["estimated_target_normals"] = True
    engine.target_fpfh(k=min(settings.feature_k, engine.n_target), keep=True, **kw_tgt)
    src_feat = fpfh(source_xyz, k=settings.feature_k, normal_k=settings.normal_k, device=engine.device, **kw_src)
    poses, frep = engine.feature_candidates(src_feat, None, n_hyp=settings.n_hyp, ratio=settings.ratio, mutual=settings.mutual,
                                            edge_tol=settings.edge_tol, seed=settings.seed)
    rep.update(("feature_" + k, v) for k, v in frep.items())
    return poses, rep


def feature_poses_downsampled(engine, settings: CoarseSettings, target_xyz, mx_base, source_xyz) -> tuple:
    """feature_poses with the descriptors taken from voxel downsamples of both clouds (settings.voxel, world units): the
    candidates are world motions applied to the incoming matrix_world and do not depend on which points produced them, so they
    suit the main engine's scoring unchanged.  Everything runs on a side engine on the same device; `engine` is only read
    (its matrix_world).  The source's cloud is ALL of source_xyz, as feature_poses computes its descriptors.
    Fewer than 4 rows on a side: no poses and rep["feature_note"] says why."""
    from .. import fpfh
    from ..engine import IcpEngine
    from .icp_align import world_scale
    mx_align = engine.matrix_world()
    h = float(settings.voxel)
    rep = {"estimated_target_normals": True, "feature_voxel": h, "feature_n_target": 0, "feature_n_source": 0, "feature_n_pairs": 0,
           "feature_n_accepted": 0}
    none = np.zeros((0, 4, 4), np.float32)
    kw_tgt, kw_src = _feature_radii(settings, mx_align, mx_base)
    with IcpEngine(engine.device) as side:
        down_tgt = side.voxel_downsample(target_xyz, h / world_scale(mx_base))["xyz"]
        down_src = side.voxel_downsample(source_xyz, h / world_scale(mx_align))["xyz"]
        rep["feature_n_target"], rep["feature_n_source"] = len(down_tgt), len(down_src)
        if len(down_tgt) < 4 or len(down_src) < 4:
            rep["feature_note"] = "%d target and %d source rows after the downsample (4 needed)" % (len(down_tgt), len(down_src))
            return none, rep
        side.set_target(down_tgt)
        side.estimate_target_normals(k=min(settings.normal_k, len(down_tgt)), orient="away", install=True, **kw_tgt)
        side.target_fpfh(k=min(settings.feature_k, len(down_tgt)), keep=True, **kw_tgt)
        src_feat = fpfh(down_src, k=settings.feature_k, normal_k=settings.normal_k, device=engine.device, **kw_src)
        side.set_source(down_src, stride=1)
        side.set_matrices(mx_align, mx_base)
        poses, frep = side.feature_candidates(src_feat, None, n_hyp=settings.n_hyp, ratio=settings.ratio, mutual=settings.mutual,
                                              edge_tol=settings.edge_tol, seed=settings.seed)
    rep.update(("feature_" + k, v) for k, v in frep.items())
    return poses, rep


def coarse_stage(engine, settings: CoarseSettings, target_xyz, mx_base, source_xyz=None) -> dict:
    """The coarse stage on an engine whose target, source and matrices are set: matrix_world moves to the pose it found.
    source_xyz: all vertices of the source, what method "features" / "both" computes the source's descriptors from.
    report["status"]: "ok", or "fallback: ..." when the features gave no candidate and (method "features") the incoming pose
    stays or (method "both") the rotations alone were scored.  Never raises for want of features."""
    thresh = settings.thresh if settings.thresh is not None else default_thresh(target_xyz, mx_base)
    kw = dict(n_refine=settings.n_refine, refine_iters=settings.refine_iters, stride=settings.stride)
    if settings.method == "rotations":
        return engine.coarse_align(thresh, n_rot=settings.n_rot, **kw)
    if source_xyz is None:
        raise ValueError("CoarseSettings.method = %r needs source_xyz" % (settings.method,))
    if settings.voxel is None:
        poses, frep = feature_poses(engine, settings, source_xyz, mx_base=mx_base)
    else:
        poses, frep = feature_poses_downsampled(engine, settings, target_xyz, mx_base, source_xyz)
    status = "ok"
    if len(poses) == 0:
        status = "fallback: no candidate from the features (%d matched pairs)" % frep["feature_n_pairs"]
        if "feature_note" in frep:
            status = "fallback: " + frep.pop("feature_note")
    if settings.method == "both":
        poses = np.concatenate([engine.coarse_candidates(settings.n_rot), poses.reshape(-1, 4, 4)])
    if len(poses) == 0:
        rep = {"n_candidates": 0, "matrix_world": engine.matrix_world()}
    else:
        rep = engine.coarse_align_poses(poses, thresh, **kw)
    rep.update(frep)
    rep["status"] = status
    rep["method"] = settings.method
    return rep


class CoarseAlign:
    """The coarse stage alone, without Blender."""

    def __init__(self, settings: CoarseSettings | None = None, engine=None):
        self.settings = settings if settings is not None else CoarseSettings()
        self.engine = engine if engine is not None else default_engine()

    def run(self, source_xyz, target_xyz, mx_align, mx_base, vlist=None, target_tris=None):
        """Returns (matrix_world float32 4x4, report dict)."""
        eng = self.engine
        if target_tris is not None:
            eng.set_target_mesh(target_xyz, target_tris)
        else:
            eng.set_target(target_xyz)
        eng.set_source(source_xyz, vlist=vlist, stride=1)
        eng.set_matrices(mx_align, mx_base)
        rep = coarse_stage(eng, self.settings, target_xyz, mx_base, source_xyz=source_xyz)
        return rep["matrix_world"], rep
