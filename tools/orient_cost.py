"""What a consistent orientation costs: oa_orient_target_normals (graph k = 8, seed away from the centroid, installed) beside
oa_estimate_target_normals (k = 16, installed) -- the call it follows -- on the same context, same build, same GPU, same run.

The cloud is a torus (R = 1, r = 0.35) of random points: the shape the orient rule of the estimate gets wrong.  Host arrays out:
the copies of the results are part of every call's time, as they are for a caller.  Each call is warmed once and timed `reps`
times with the host's clock around it (both end in a device synchronisation); the least time is reported, with the merging rounds
and the components the orientation found and the share of normals that then agree with the analytic ones.  Prints one JSON line.
No pass/fail bar: DESIGN.md 3.22 records the numbers.

    python tools/orient_cost.py [--sizes 100000,1000000] [--k 8] [--normal-k 16] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from object_alignment_amd.engine import IcpEngine           # noqa: E402


def torus(n, R=1.0, r=0.35, seed=1):
    """n random points of a torus and its analytic outward normals."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    xyz = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], 1)
    return xyz.astype(np.float32), np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)


def least_ms(call, reps):
    call()                                                      # warm: code objects, the allocation cache
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def leg(e, n, k, normal_k, reps):
    xyz, analytic = torus(n)
    e.set_target(xyz)
    est = e.estimate_target_normals(k=normal_k, orient="away", install=True)[0]
    nrm, flipped, comp, rep = e.orient_target_normals(k=k, install=True)
    agree = lambda a: round(float(np.mean(np.einsum("ij,ij->i", a.astype(np.float64), analytic) > 0)), 5)       # noqa: E731
    out = {"n": n, "k": k, "normal_k": normal_k, "rounds": rep["rounds"], "components": rep["n_components"], "left_out": rep["n_left_out"],
           "flipped": rep["n_flipped"], "agree_away": agree(est), "agree_consistent": agree(nrm)}
    out["estimate_target_normals_ms"] = round(least_ms(lambda: e.estimate_target_normals(k=normal_k, orient="away", install=True), reps), 3)
    out["orient_target_normals_ms"] = round(least_ms(lambda: e.orient_target_normals(k=k, install=True), reps), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--normal-k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    res = {"reps": args.reps, "legs": []}
    with IcpEngine(args.device) as e:
        for n in (int(t) for t in args.sizes.split(",")):
            res["legs"].append(leg(e, n, args.k, args.normal_k, args.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
