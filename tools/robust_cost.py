"""What a weighted loop costs per iteration: loss none against Tukey at a fixed scale against Tukey with the scale taken
from each step's residuals (oa_set_robust_auto: the median, times MAD_TUNING["tukey"]), same build, same GPU, same inputs.

A weighted step runs search -> accumulate (no accumulating search epilogue knows about weights), so besides the weighted
accumulation itself it gives up the fused epilogue of the grid and tree searches.  The estimated scale adds a read-only pair
fetch, the radix select over the 4-byte keys and its scans (six launches) between the search and the weighted accumulation.
Two legs, each timed as loop_ms / iters_done of a loop that cannot end early:
  point  1M <-> 1M random clouds (bench.py's flagship inputs), grid search, point metric
  plane  1M bunny points on the 1.96M-triangle lattice mesh (bench.py's surface leg), plane metric
Prints one JSON line.  No pass/fail bar: DESIGN.md 3.10 records the numbers.

    python tools/robust_cost.py [--n 1000000] [--steps 30] [--scale 0.05]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from object_alignment_amd import synth                      # noqa: E402
from object_alignment_amd.engine import IcpEngine           # noqa: E402
from object_alignment_amd.operators.icp_align import MAD_TUNING   # noqa: E402


def per_iteration_ms(e, steps, warmup, mxa, mxb, reps=3):
    best = None
    for rep in range(warmup + reps):
        e.set_matrices(mxa, mxb)
        r = e.run(iters=steps, thresh=0.5, target_d=0.0, early_exit=False)
        if rep >= warmup:
            ms = r.loop_ms / max(1, r.iters_done)
            best = ms if best is None else min(best, ms)
    return best, r


def leg(e, steps, scale, mxa, mxb):
    out = {}
    for name in ("none", "tukey", "tukey_auto"):
        e.set_robust("none" if name == "none" else "tukey", {"none": 0.0, "tukey": scale, "tukey_auto": MAD_TUNING["tukey"]}[name])
        e.set_robust_auto(0.5 if name == "tukey_auto" else 0.0, 1e-4)
        ms, r = per_iteration_ms(e, steps, 1, mxa, mxb)
        out[name] = {"ms_per_iteration": round(ms, 4), "iters": r.iters_done, "last_K": r.last_K, "weight_sum": e.stat("weight_sum"),
                     "robust_scale": e.stat("robust_scale"), "fast_iterations": int(e.stat("fast_iterations"))}
    e.set_robust_auto(0.0)
    out["tukey_over_none"] = round(out["tukey"]["ms_per_iteration"] / out["none"]["ms_per_iteration"], 3)
    out["auto_over_fixed"] = round(out["tukey_auto"]["ms_per_iteration"] / out["tukey"]["ms_per_iteration"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--scale", type=float, default=0.05)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    res = {"n": args.n, "steps": args.steps, "scale": args.scale}
    src, tgt, mxa, mxb = synth.c3_random_pair(args.n, seed=1234, n_target=args.n)
    with IcpEngine(args.device) as e:
        e.set_search_mode("grid")
        e.set_target(tgt)
        e.set_source(src, stride=1)
        res["point_grid"] = leg(e, args.steps, args.scale, mxa, mxb)
    verts, tris = synth.lattice_surface_mesh(700, 1400) if args.n >= 1_000_000 else synth.cubed_surface_mesh(40)
    pts = synth.bunny_surface(args.n, offset=0.37)
    s_mxa = synth.rigid4(synth.rotation_from_rotvec([0.02, -0.015, 0.025]), [0.01, -0.008, 0.012])
    with IcpEngine(args.device) as e:
        e.set_metric("plane")
        e.set_target_mesh(verts, tris)
        e.set_source(pts, stride=1)
        res["plane_surface"] = dict(leg(e, args.steps, args.scale, s_mxa, np.identity(4, dtype=np.float32)), n_tris=int(len(tris)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
