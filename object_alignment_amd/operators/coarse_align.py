"""Coarse global alignment in front of the ICP loop (no counterpart in the reference, whose remedy for a bad start is picking
landmarks by hand, operators/align_pick_points.py).

`CoarseAlign.run` is "align these two scans" without landmarks: a few hundred candidate poses -- the source turned about its
centroid by a super-Fibonacci set of rotations, centroid on centroid -- are scored on the GPU in one launch by the truncated mean
distance of a sample to the target, the best few get a short point loop, and the cheapest becomes matrix_world
(oa_coarse_align).  `IcpAlign.run(..., coarse=CoarseSettings())` runs it on the same engine in front of the usual loop.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ..functions.general import default_engine

THRESH_FRACTION = 0.1       # thresh=None: this part of the target's world-space bounding-box diagonal


@dataclass
class CoarseSettings:
    n_rot: int = 256                # rotation candidates
    n_refine: int = 8               # best candidates that get a short loop
    refine_iters: int = 10          # iterations of that loop
    stride: int = 4                 # every stride-th point of the selection is scored and refined
    thresh: float | None = None     # truncation / pair distance, world units; None = THRESH_FRACTION x the target's diagonal

    def __post_init__(self):
        for name, lo, hi in (("n_rot", 1, 65536), ("n_refine", 1, 4096), ("refine_iters", 0, 10000), ("stride", 1, 1 << 30)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError("CoarseSettings.%s = %r (an integer in %d .. %d)" % (name, v, lo, hi))
        if self.thresh is not None and not (np.isfinite(self.thresh) and self.thresh > 0):
            raise ValueError("CoarseSettings.thresh = %r (finite and > 0, or None)" % (self.thresh,))


def default_thresh(target_xyz, mx_base) -> float:
    """THRESH_FRACTION x the diagonal of the target's axis-aligned bounding box in world space."""
    t = np.asarray(target_xyz, np.float64).reshape(-1, 3)
    m = np.asarray(mx_base, np.float64).reshape(4, 4)
    w = t @ m[:3, :3].T + m[:3, 3]
    w = w[np.all(np.isfinite(w), axis=1)]
    if len(w) == 0:
        raise ValueError("the target has no finite vertex")
    return THRESH_FRACTION * float(np.linalg.norm(w.max(axis=0) - w.min(axis=0)))


def coarse_stage(engine, settings: CoarseSettings, target_xyz, mx_base) -> dict:
    """The coarse stage on an engine whose target, source and matrices are set: matrix_world moves to the pose it found."""
    thresh = settings.thresh if settings.thresh is not None else default_thresh(target_xyz, mx_base)
    return engine.coarse_align(thresh, n_rot=settings.n_rot, n_refine=settings.n_refine, refine_iters=settings.refine_iters,
                               stride=settings.stride)


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
        rep = coarse_stage(eng, self.settings, target_xyz, mx_base)
        return rep["matrix_world"], rep
