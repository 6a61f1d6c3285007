"""What the coarse stage costs: oa_score_poses for P poses in one launch against the same scores through the
interface the library had before it -- oa_set_matrices + oa_make_pairs(calc_stats=1) per pose, same build, same GPU, same
inputs -- and the whole oa_coarse_align call next to the 50-iteration loop that follows it.

One GPU process; every step runs in a child process of its own under its own time limit (--step runs one of them).  Times are
host clocks around calls that end in a device synchronise, best of --reps after a warm-up.  Prints one JSON line.  No pass/fail
bar.

    python tools/coarse_cost.py [--n 100000] [--poses 257] [--stride 4] [--reps 3]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"score": 300, "align": 300}          # step -> its time limit in seconds


def inputs(n):
    from object_alignment_amd import synth
    tgt = synth.bunny_surface(n, 0.0)
    src = synth.bunny_surface(n, 0.37)
    start = synth.rigid4(synth.rotation_from_rotvec([2.4, 0.3, -0.5]), [0.4, -0.3, 0.25])
    return src, tgt, start, np.identity(4, dtype=np.float32)


def best_ms(f, reps):
    f()                                       # warm-up: code objects, the allocation cache
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return best


def step_score(args):
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.coarse_align import default_thresh
    src, tgt, start, eye = inputs(args.n)
    thresh = default_thresh(tgt, eye)
    out = {"thresh": thresh}
    with IcpEngine(args.device) as e:
        e.set_target(tgt)
        e.set_source(src, stride=1)
        e.set_matrices(start, eye)
        poses = np.concatenate([e.coarse_candidates(args.poses - 1), start[None]])
        out["sample_points"] = -(-len(src) // args.stride)
        out["score_poses_ms"] = best_ms(lambda: e.score_poses(poses, thresh, args.stride), args.reps)
        batched = e.score_poses(poses, thresh, args.stride)
    with IcpEngine(args.device) as e:         # the interface before: the strided selection as the source, one pose per call
        e.set_target(tgt)
        e.set_source(src, stride=args.stride)
        single = np.empty((len(poses), 3))

        def per_pose():
            for p, M in enumerate(poses):
                e.set_matrices(M, eye)
                A, _, ds = e.make_pairs(thresh, calc_stats=True)
                single[p] = [A.shape[1], ds[0], ds[1]]
        out["make_pairs_per_pose_ms"] = best_ms(per_pose, args.reps)
    ok = ~np.isnan(single[:, 1])
    out["same_K"] = bool(np.array_equal(single[:, 0], batched[:, 0]))
    out["mean_max_rel_diff"] = float(np.max(np.abs(single[ok, 1] - batched[ok, 1]) / np.abs(single[ok, 1]))) if ok.any() else 0.0
    out["ratio"] = out["make_pairs_per_pose_ms"] / out["score_poses_ms"]
    return out


def step_align(args):
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.coarse_align import default_thresh
    src, tgt, start, eye = inputs(args.n)
    thresh = default_thresh(tgt, eye)
    out = {}
    with IcpEngine(args.device) as e:
        e.set_target(tgt)
        e.set_source(src, stride=1)
        reports = []

        def coarse():
            e.set_matrices(start, eye)
            reports.append(e.coarse_align(thresh, n_rot=args.poses - 1, stride=args.stride))
        out["coarse_align_ms"] = best_ms(coarse, args.reps)
        rep = reports[-1]
        out["report"] = {k: v for k, v in rep.items() if k != "matrix_world"}
        runs = []

        def loop():
            e.set_matrices(rep["matrix_world"], eye)
            runs.append(e.run(iters=50, thresh=0.5, early_exit=False))
        out["loop_50_ms"] = best_ms(loop, args.reps)
        out["loop_50_device_ms"] = runs[-1].loop_ms
        M = runs[-1].matrix_world.astype(np.float64)
        out["final_angle_deg"] = float(np.degrees(np.arccos(np.clip((np.trace(M[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))))
    out["coarse_over_loop"] = out["coarse_align_ms"] / out["loop_50_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--poses", type=int, default=257)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--step", choices=sorted(STEPS))
    args = ap.parse_args()
    if args.step:
        print(json.dumps({"score": step_score, "align": step_align}[args.step](args)))
        return 0
    res = {"n": args.n, "poses": args.poses, "stride": args.stride}
    for step in ("score", "align"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--n", str(args.n), "--poses", str(args.poses),
               "--stride", str(args.stride), "--reps", str(args.reps), "--device", str(args.device)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[step])
        except subprocess.TimeoutExpired:
            res[step] = "timed out after %d s" % STEPS[step]
            break                             # nothing more is started on a GPU that did not answer
        if p.returncode != 0:
            res[step] = "exit status %d: %s" % (p.returncode, p.stderr[-400:])
            break
        res[step] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    return 0 if all(isinstance(res.get(s), dict) for s in STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
