"""What the trim costs per iteration: the same loop with oa_set_trim off, with a fixed share and with the estimated share, same
build, same GPU, same inputs.

A trimmed step runs search -> trim -> accumulate and gives up the fused epilogue of the grid and tree searches, as a weighted
step does -- so beside the plain loop ("off") the yardstick is the plain WEIGHTED step of the same commit (Huber at c = 1e30:
every weight is one, search + k_pair_accumulate_weighted as separate launches).  trim_ms = a trimmed step minus that one: the
trim's own launches (fixed share: keys, two histograms, three scans of the radix select, the verdict; estimated share: keys, the
32-bit sort and gather, tile sums, tile bases, apply, argmin, the verdict; two memsets either way) plus the RECIP variant of the
accumulation reading one byte per slot.
Legs, each timed as loop_ms / iters_done of a loop that cannot end early, grid search, point metric:
  c2   100k <-> 100k bunny points (BASELINE's configuration 2)
  1m   1M <-> 1M random clouds (bench.py's flagship inputs)
Prints one JSON line.  No pass/fail bar: DESIGN.md 3.18 records the numbers.

    python tools/trim_cost.py [--steps 30] [--legs c2,1m]
"""
import argparse
import json
import os
import sys

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
    for name, trim, loss in (("off", 0.0, None), ("weighted", 0.0, "huber"), ("fixed_0.5", 0.5, None), ("estimated", "auto", None)):
        e.set_trim(trim)
        e.set_robust(loss or "none", 1e30 if loss else 0.0)
        ms, r = per_iteration_ms(e, steps, 1, mxa, mxb)
        out[name] = {"ms_per_iteration": round(ms, 4), "iters": r.iters_done, "last_K": r.last_K,
                     "candidates_last_step": int(e.stat("trim_candidates")), "kept_last_step": int(e.stat("trim_kept")),
                     "fast_iterations": int(e.stat("fast_iterations"))}
    e.set_trim(0.0)
    e.set_robust("none")
    for name in ("fixed_0.5", "estimated"):
        out[name]["trim_ms"] = round(out[name]["ms_per_iteration"] - out["weighted"]["ms_per_iteration"], 4)
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
