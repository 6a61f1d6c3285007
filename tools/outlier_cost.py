"""What outlier removal costs: oa_target_outliers -- (a) statistical with k = 16, (b) radius at a radius that holds about 16
neighbours, with exact counts and with count_cap = min_neighbors + 1 -- beside (c) oa_target_knn(k = 17) with both host outputs,
the only other route to the statistical score, on the same context, same build, same GPU, same run.

The cloud is a torus (R = 1, r = 0.35) of random points plus 1 % strays, uniform in the box [-2, 2] x [-2, 2] x [-0.6, 0.6].
Nothing is applied: every call sees the same target.  Host arrays out: the copies of the results are part of every call's time,
as they are for a caller.  Each call is warmed once and timed `reps` times with the host's clock around it (all end in a device
synchronisation); the least time is reported, for (c) also the largest -- its run-to-run spread is what (a) is read against.
Prints one JSON line.  No pass/fail bar: DESIGN.md 3.23 records the numbers.

    python tools/outlier_cost.py [--sizes 100000,1000000] [--k 16] [--min-neighbors 8] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from object_alignment_amd.engine import IcpEngine           # noqa: E402

TORUS_R, TORUS_r = 1.0, 0.35


def cloud(n, seed=1):
    """n random points of the torus and n / 100 strays, shuffled."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    xyz = np.stack([(TORUS_R + TORUS_r * np.cos(v)) * np.cos(u), (TORUS_R + TORUS_r * np.cos(v)) * np.sin(u), TORUS_r * np.sin(v)], 1)
    stray = rng.uniform([-2, -2, -0.6], [2, 2, 0.6], (n // 100, 3))
    pts = np.concatenate([xyz, stray]).astype(np.float32)
    perm = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), perm < n


def times_ms(call, reps):
    call()                                                      # warm: code objects, the allocation cache
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def leg(e, n, k, min_neighbors, reps):
    xyz, surface = cloud(n)
    e.set_target(xyz)
    # a disc of this radius on the surface holds about 16 points: pi radius^2 n / (4 pi^2 R r) = 16
    radius = float(np.sqrt(16.0 * 4.0 * np.pi * TORUS_R * TORUS_r / n))
    stat = e.target_outliers(method="statistical", k=k, std_ratio=2.0)
    rad = e.target_outliers(method="radius", radius=radius, min_neighbors=min_neighbors)
    share = lambda keep: [round(float(keep[surface].mean()), 5), round(float(1.0 - keep[~surface].mean()), 5)]      # noqa: E731
    out = {"n": len(xyz), "k": k, "radius": round(radius, 6), "min_neighbors": min_neighbors,
           "mean_count": round(float(rad["count"][surface].mean()), 2),
           "statistical_surface_kept_strays_removed": share(stat["keep"].astype(bool)),
           "radius_surface_kept_strays_removed": share(rad["keep"].astype(bool))}
    ms = lambda t: round(min(t), 3)                                                                                  # noqa: E731
    out["a_outliers_statistical_ms"] = ms(times_ms(lambda: e.target_outliers(method="statistical", k=k, std_ratio=2.0), reps))
    out["b_outliers_radius_exact_ms"] = ms(times_ms(lambda: e.target_outliers(method="radius", radius=radius, min_neighbors=min_neighbors), reps))
    out["b_outliers_radius_capped_ms"] = ms(times_ms(lambda: e.target_outliers(method="radius", radius=radius, min_neighbors=min_neighbors,
                                                                               count_cap=min_neighbors + 1), reps))
    out["radius_count_exact_ms"] = ms(times_ms(lambda: e.target_radius_count(radius), reps))
    c = times_ms(lambda: e.target_knn(k + 1), reps)
    out["c_target_knn_ms"], out["c_target_knn_max_ms"] = ms(c), round(max(c), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--min-neighbors", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    res = {"reps": args.reps, "legs": []}
    with IcpEngine(args.device) as e:
        for n in (int(t) for t in args.sizes.split(",")):
            res["legs"].append(leg(e, n, args.k, args.min_neighbors, args.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
