"""What rejecting boundary pairs costs per iteration: the same loop with oa_set_reject_boundary off and on, same build, same GPU,
same inputs, plus the one-off build of the target's boundary masks.

A step with the setting on runs search -> k_boundary_verdict -> accumulate: a memset of the verdict bytes, one thread per slot
(a table lookup in vertex mode, closest_on_tri_region and a lookup in surface mode) and the RECIP variant of the accumulation; it
gives up the fused epilogue of the grid and tree searches, as a weighted step does.  So beside the plain loop ("off") the
yardsticks are the plain WEIGHTED step of the same commit (Huber at c = 1e30: every weight is one, search +
k_pair_accumulate_weighted as separate launches; tools/trim_cost.py's) and the reciprocal check (tools/recip_cost.py's).
Legs, each timed as loop_ms / iters_done of a loop that cannot end early, best of 3, grid search, point metric:
  c2     100k <-> 100k bunny points (BASELINE's configuration 2), estimated target normals
  1m     1M <-> 1M random clouds (bench.py's flagship inputs), estimated target normals
  mesh   200k points on the 82k-triangle mesh (surface mode)
mask_build_ms: wall time of the first target_boundary call (k-nearest rows + the angle criterion, or corner rows + the edge walk).
Prints one JSON line.  No pass/fail bar: DESIGN.md 3.19 records the numbers.

    python tools/boundary_cost.py [--steps 30] [--legs c2,1m,mesh]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from object_alignment_amd import synth                      # noqa: E402
from object_alignment_amd.engine import IcpEngine           # noqa: E402


def per_iteration_ms(e, steps, warmup, mxa, mxb, thresh, reps=3):
    best = None
    for rep in range(warmup + reps):
        e.set_matrices(mxa, mxb)
        r = e.run(iters=steps, thresh=thresh, target_d=0.0, early_exit=False)
        if rep >= warmup:
            ms = r.loop_ms / max(1, r.iters_done)
            best = ms if best is None else min(best, ms)
    return best, r


def leg(e, steps, mxa, mxb, thresh):
    out = {}
    t0 = time.perf_counter()
    vm, em = e.target_boundary()
    out["mask_build_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    t0 = time.perf_counter()
    e.target_boundary()
    out["mask_copy_ms"] = round((time.perf_counter() - t0) * 1e3, 3)                 # (the second call finds them built)
    out["boundary_vertices"], out["boundary_edges"] = int(e.stat("boundary_vertices")), int(e.stat("boundary_edges"))
    for name, bnd, recip, loss in (("off", False, False, None), ("weighted", False, False, "huber"), ("boundary", True, False, None),
                                   ("reciprocal", False, True, None)):
        e.set_reject_boundary(bnd)
        e.set_reciprocal(recip)
        e.set_robust(loss or "none", 1e30 if loss else 0.0)
        ms, r = per_iteration_ms(e, steps, 1, mxa, mxb, thresh)
        out[name] = {"ms_per_iteration": round(ms, 4), "iters": r.iters_done, "last_K": r.last_K,
                     "boundary_rejected_last_step": int(e.stat("boundary_rejected")), "recip_rejected_last_step": int(e.stat("recip_rejected")),
                     "fast_iterations": int(e.stat("fast_iterations"))}
    e.set_reject_boundary(False)
    e.set_reciprocal(False)
    e.set_robust("none")
    out["boundary_minus_weighted_ms"] = round(out["boundary"]["ms_per_iteration"] - out["weighted"]["ms_per_iteration"], 4)
    out["reciprocal_minus_weighted_ms"] = round(out["reciprocal"]["ms_per_iteration"] - out["weighted"]["ms_per_iteration"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--legs", default="c2,1m,mesh")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    res = {"steps": args.steps}
    for name in args.legs.split(","):
        tris, thresh = None, 0.5
        if name == "c2":
            src, tgt, mxa, mxb = synth.c2_bunny_pair(100_000)
        elif name == "1m":
            src, tgt, mxa, mxb = synth.c3_random_pair(1_000_000, seed=1234, n_target=1_000_000)
        elif name == "mesh":
            tgt, tris = synth.bumpy_icosphere_mesh(6)
            src = synth.bunny_surface(200_000, offset=0.37)
            mxa = synth.rigid4(synth.rotation_from_rotvec([0.02, -0.015, 0.025]), [0.01, -0.008, 0.012])
            mxb, thresh = np.identity(4, dtype=np.float32), 0.05
        else:
            raise SystemExit("unknown leg %r (c2, 1m, mesh)" % name)
        with IcpEngine(args.device) as e:
            e.set_search_mode("grid")
            if tris is None:
                e.set_target(tgt)
                e.estimate_target_normals(k=16, orient="none", install=True)
            else:
                e.set_target_mesh(tgt, tris)
            e.set_source(src, stride=1)
            res[name] = dict(leg(e, args.steps, mxa, mxb, thresh), n_source=int(len(src)), n_target=int(len(tgt)),
                             n_tris=0 if tris is None else int(len(tris)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
