"""What the feature-based coarse stage costs, stage by stage, beside oa_coarse_align on the same build, the same
GPU and the same inputs: a half of one n-point sampling of the synthetic bunny against another full n-point sampling.

One GPU process; every step runs in a child process of its own under its own time limit (--step runs one of them).  Times are
host clocks around calls that end in a device synchronise, best of --reps after a warm-up.  Prints one JSON line.  No pass/fail
bar.

    python tools/feature_cost.py [--n 100000] [--k 16] [--reps 3]
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

STEPS = {"features": 600, "rotations": 300}          # step -> its time limit in seconds


def inputs(n):
    from object_alignment_amd import synth
    tgt = synth.bunny_surface(n, 0.0)
    full = synth.bunny_surface(2 * n, 0.37)
    src = np.ascontiguousarray(full[full[:, 0] > 0.0][:n])
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


def angle_deg(M):
    M = np.asarray(M, np.float64)
    return float(np.degrees(np.arccos(np.clip((np.trace(M[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))))


def step_features(args):
    import object_alignment_amd as oa
    from object_alignment_amd.engine import IcpEngine
    from object_alignment_amd.operators.coarse_align import default_thresh
    src, tgt, start, eye = inputs(args.n)
    thresh = default_thresh(tgt, eye)
    out = {"n_source": len(src), "n_target": len(tgt)}
    with IcpEngine(args.device) as e:
        e.set_target(tgt)
        e.set_source(src, stride=1)
        e.set_matrices(start, eye)
        out["target_normals_ms"] = best_ms(lambda: e.estimate_target_normals(k=args.k, orient="away", install=True), args.reps)
        out["target_fpfh_ms"] = best_ms(lambda: e.target_fpfh(k=args.k, keep=True), args.reps)
        out["source_fpfh_own_context_ms"] = best_ms(lambda: oa.fpfh(src, k=args.k, normal_k=args.k, device=args.device), args.reps)
        sf, tf = oa.fpfh(src, k=args.k, normal_k=args.k, device=args.device), e.target_fpfh(k=args.k, keep=True)
        out["match_one_direction_ms"] = best_ms(lambda: e.match_features(sf, tf), args.reps)
        got = []
        out["feature_candidates_ms"] = best_ms(lambda: got.append(e.feature_candidates(sf, None)), args.reps)
        poses, frep = got[-1]
        out["feature_report"] = frep
        if len(poses):
            reports = []

            def align():
                e.set_matrices(start, eye)
                reports.append(e.coarse_align_poses(poses, thresh))
            out["coarse_align_poses_ms"] = best_ms(align, args.reps)
            out["coarse_report"] = {k: v for k, v in reports[-1].items() if k != "matrix_world"}
            e.set_matrices(reports[-1]["matrix_world"], eye)
            out["final_angle_deg"] = angle_deg(e.run(iters=50, thresh=0.5, early_exit=False).matrix_world)
    return out


def step_rotations(args):
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
            reports.append(e.coarse_align(thresh))
        out["coarse_align_ms"] = best_ms(coarse, args.reps)
        e.set_matrices(reports[-1]["matrix_world"], eye)
        out["final_angle_deg"] = angle_deg(e.run(iters=50, thresh=0.5, early_exit=False).matrix_world)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--step", choices=sorted(STEPS))
    args = ap.parse_args()
    if args.step:
        print(json.dumps({"features": step_features, "rotations": step_rotations}[args.step](args)))
        return 0
    res = {"n": args.n, "k": args.k}
    for step in ("features", "rotations"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--n", str(args.n), "--k", str(args.k),
               "--reps", str(args.reps), "--device", str(args.device)]
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
