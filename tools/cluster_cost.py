"""What clustering costs: oa_target_clusters (eps = a radius that holds about 16 neighbours, min_points 8, keep the largest) beside
oa_target_radius_count uncapped and capped at min_points, and oa_target_outliers (radius) -- the same context, same build, same GPU,
same run.

The cloud is tools/outlier_cost.py's: a torus (R = 1, r = 0.35) of random points plus 1 % strays.  Nothing is applied: every call
sees the same target.  Host arrays out: the copies of the results are part of every call's time, as they are for a caller.  Each
call is warmed once and timed `reps` times with the host's clock around it (all end in a device synchronisation); the least time is
reported.  Prints one JSON line.  No pass/fail bar: DESIGN.md 3.24 records the numbers.

    python tools/cluster_cost.py [--sizes 100000,1000000] [--min-points 8] [--reps 5]

The passes inside the call -- the capped count, the link pass, the flatten, the border pass -- are kernels of one stream; their times
come from a kernel trace of this same script, read back with --kernels:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/cluster_cost.py --sizes 1000000 --reps 3
    python tools/cluster_cost.py --kernels DIR
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TORUS_R, TORUS_r = 1.0, 0.35
PASSES = (("count_capped", "k_bvh_radius_count<true>"), ("count_exact", "k_bvh_radius_count<false>"), ("link", "k_bvh_cluster<0>"),
          ("flatten", "k_cluster_flatten"), ("border", "k_bvh_cluster<1>"), ("label", "k_cluster_label"), ("largest", "k_cluster_largest"),
          ("keep", "k_cluster_keep"), ("compact", "k_outlier_compact"))


def cloud(n, seed=1):
    """n random points of the torus and n / 100 strays, shuffled."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    xyz = np.stack([(TORUS_R + TORUS_r * np.cos(v)) * np.cos(u), (TORUS_R + TORUS_r * np.cos(v)) * np.sin(u), TORUS_r * np.sin(v)], 1)
    stray = rng.uniform([-2, -2, -0.6], [2, 2, 0.6], (n // 100, 3))
    pts = np.concatenate([xyz, stray]).astype(np.float32)
    perm = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), perm < n


def least_ms(call, reps):
    call()                                                      # warm: code objects, the allocation cache
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(min(t), 3)


def leg(e, n, min_points, reps):
    xyz, surface = cloud(n)
    e.set_target(xyz)
    # a disc of this radius on the surface holds about 16 points: pi radius^2 n / (4 pi^2 R r) = 16
    eps = float(np.sqrt(16.0 * 4.0 * np.pi * TORUS_R * TORUS_r / n))
    out = e.target_clusters(eps, min_points=min_points, keep="largest")
    rep = out["report"]
    keep = out["keep"].astype(bool)
    res = {"n": len(xyz), "eps": round(eps, 6), "min_points": min_points,
           "report": rep, "surface_kept_strays_removed": [round(float(keep[surface].mean()), 5), round(float(1.0 - keep[~surface].mean()), 5)]}
    res["clusters_ms"] = least_ms(lambda: e.target_clusters(eps, min_points=min_points, keep="largest"), reps)
    res["radius_count_exact_ms"] = least_ms(lambda: e.target_radius_count(eps), reps)
    res["radius_count_capped_ms"] = least_ms(lambda: e.target_radius_count(eps, min_points), reps)
    res["outliers_radius_ms"] = least_ms(lambda: e.target_outliers(method="radius", radius=eps, min_neighbors=min_points), reps)
    return res


def kernels(d):
    """the least and the median time of every pass's kernel in the newest kernel trace under d, in microseconds, at the LARGEST
    grid each was launched with (the last size of --sizes)"""
    f = sorted(glob.glob(d + "/**/*_kernel_trace.csv", recursive=True))[-1]
    rows = list(csv.DictReader(open(f)))
    out = {}
    for name, pattern in PASSES:
        mine = [r for r in rows if pattern in r["Kernel_Name"]]
        if not mine:
            continue
        grid = max(int(r["Grid_Size"]) for r in mine) if "Grid_Size" in mine[0] else None
        t = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine if grid is None or int(r["Grid_Size"]) == grid)
        out[name] = {"kernel": pattern, "launches": len(t), "least_us": round(t[0], 1), "median_us": round(t[len(t) // 2], 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--min-points", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--kernels", metavar="DIR", help="read a kernel trace of this script instead of running")
    args = ap.parse_args()
    if args.kernels:
        print(json.dumps({"kernels": kernels(args.kernels)}))
        return
    from object_alignment_amd.engine import IcpEngine
    res = {"reps": args.reps, "legs": []}
    with IcpEngine(args.device) as e:
        for n in (int(t) for t in args.sizes.split(",")):
            res["legs"].append(leg(e, n, args.min_points, args.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
