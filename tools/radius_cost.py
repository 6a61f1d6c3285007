"""What a neighbour radius costs: per-launch times of k_bvh_knn (k = 16, a 1M-point cloud) with the radius off and at 2, 4 and 8 x
the cloud's spacing -- the same context, same build, same GPU, same run.

The cloud is tools/outlier_cost.py's torus (R = 1, r = 0.35) of random points, without the strays.  Two launches are timed per
setting: oa_target_knn with both outputs NULL (k_bvh_knn<false>: the search alone, no row leaves the device) and
oa_estimate_target_normals installing its result (k_bvh_knn<true>: the search and the 64-wide eigen-solves).  Each is warmed once
and timed `reps` times with the host's clock around it (both end in a device synchronisation); the least and the median time are
reported, and the settings are visited in turn, `rounds` times over, so that a drift of the clock hits all of them alike.  A library
without oa_set_neighbor_radius (this script copied into a built checkout of an older commit and run there) is timed with the
radius off alone: that is how the off path is held against its predecessor -- run the two in turn, several times each.  Prints one
JSON line.  No pass/fail bar: DESIGN.md 3.25 records the numbers.

    python tools/radius_cost.py [--n 1000000] [--k 16] [--reps 10] [--rounds 3] [--multiples 2,4,8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TORUS_R, TORUS_r = 1.0, 0.35


def cloud(n, seed=1):
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    return np.stack([(TORUS_R + TORUS_r * np.cos(v)) * np.cos(u), (TORUS_R + TORUS_r * np.cos(v)) * np.sin(u), TORUS_r * np.sin(v)], 1).astype(np.float32)


def times_ms(call, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--multiples", default="2,4,8")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    from object_alignment_amd.engine import IcpEngine
    with IcpEngine(args.device) as e:
        L, h = e._L, e._h
        has_radius = hasattr(L, "oa_set_neighbor_radius")
        e.set_target(cloud(args.n))

        def knn():
            e._chk(L.oa_target_knn(h, args.k, None, None))

        def normals():
            e._chk(L.oa_estimate_target_normals(h, args.k, 0, None, 1, None, None))

        res = {"n": args.n, "k": args.k, "reps": args.reps, "rounds": args.rounds, "has_radius": has_radius, "settings": []}
        settings = [("off", 0.0)]
        if has_radius:
            spacing = e.target_spacing()
            res["spacing"] = spacing
            settings += [("%gx" % m, m * spacing["mean"]) for m in (float(t) for t in args.multiples.split(","))]
        acc = {name: {"knn": [], "normals": []} for name, _ in settings}
        for rnd in range(args.rounds + 1):                          # round 0 warms every setting: code objects, the allocation cache
            for name, r in settings:
                if has_radius:
                    e.set_neighbor_radius(r)
                a, b = times_ms(knn, 1 if rnd == 0 else args.reps), times_ms(normals, 1 if rnd == 0 else args.reps)
                if rnd > 0:
                    acc[name]["knn"] += a
                    acc[name]["normals"] += b
        for name, r in settings:
            row = {"setting": name, "radius": round(r, 9)}
            if has_radius and r > 0:
                e.set_neighbor_radius(r)
                row["mean_row_length"] = round(float((e.target_knn(args.k)[0][:: max(1, args.n // 20000)] >= 0).sum(axis=1).mean()), 3)
            for what in ("knn", "normals"):
                t = sorted(acc[name][what])
                row[what + "_ms"] = {"least": round(t[0], 3), "median": round(t[len(t) // 2], 3), "most": round(t[-1], 3)}
            res["settings"].append(row)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
