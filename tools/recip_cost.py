"""What the reciprocal check costs per iteration: the same loop with oa_set_reciprocal off and on, same build, same GPU, same
inputs, plus the one-off build of the source's box tree.

A step with the check on runs search -> k_recip_check -> accumulate: besides the check itself (one wave per slot through the
tree over the selected source points) it gives up the fused epilogue of the grid and tree searches, as a weighted step does.
Two legs, each timed as loop_ms / iters_done of a loop that cannot end early, grid search, point metric:
  c2   100k <-> 100k bunny points (BASELINE's configuration 2)
  1m   1M <-> 1M random clouds (bench.py's flagship inputs)
tree_build_ms: wall time of the first make_pairs with the check on (which builds the tree) minus that of the second (which
finds it built).  Prints one JSON line.  No pass/fail bar: DESIGN.md 3.17 records the numbers.

    python tools/recip_cost.py [--steps 30] [--legs c2,1m]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from object_alignment_amd import synth                      # noqa: E402
from object_alignment_amd.engine import IcpEngine           # noqa: E402


def per_iteration_ms(e, steps, warmup, mxa, mxb, reps=3):
    best = None
    for rep in range(warmup + reps):
        e.set_matrices(mxa, mxb)
        r = e.run(iters=steps, thresh=0.5, target_d=0.0, early_exit=False)
        if rep >= warmup:
            ms = r.loop_ms / max(1, r.iters_done)
            best = ms if best is None else min(best, ms)
    return best, r


def leg(e, steps, mxa, mxb):
    out = {}
    e.set_reciprocal(True)
    e.set_matrices(mxa, mxb)
    wall = []
    for _ in range(2):                                          # the first call builds the source tree
        t0 = time.perf_counter()
        e.make_pairs(0.5)
        wall.append((time.perf_counter() - t0) * 1e3)
    out["tree_build_ms"] = round(wall[0] - wall[1], 3)
    out["make_pairs_ms"] = round(wall[1], 3)
    for name in ("off", "on"):
        e.set_reciprocal(name == "on")
        ms, r = per_iteration_ms(e, steps, 1, mxa, mxb)
        out[name] = {"ms_per_iteration": round(ms, 4), "iters": r.iters_done, "last_K": r.last_K,
                     "rejected_last_step": int(e.stat("recip_rejected")), "fast_iterations": int(e.stat("fast_iterations"))}
    e.set_reciprocal(False)
    out["on_over_off"] = round(out["on"]["ms_per_iteration"] / out["off"]["ms_per_iteration"], 3)
    out["check_ms"] = round(out["on"]["ms_per_iteration"] - out["off"]["ms_per_iteration"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--legs", default="c2,1m")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    res = {"steps": args.steps}
    for name in args.legs.split(","):
        if name == "c2":
            src, tgt, mxa, mxb = synth.c2_bunny_pair(100_000)
        elif name == "1m":
            src, tgt, mxa, mxb = synth.c3_random_pair(1_000_000, seed=1234, n_target=1_000_000)
        else:
            raise SystemExit("unknown leg %r (c2, 1m)" % name)
        with IcpEngine(args.device) as e:
            e.set_search_mode("grid")
            e.set_target(tgt)
            e.set_source(src, stride=1)
            res[name] = dict(leg(e, args.steps, mxa, mxb), n_source=int(len(src)), n_target=int(len(tgt)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
