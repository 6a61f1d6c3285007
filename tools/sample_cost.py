"""What the selection calls cost: oa_normal_space_sample (m = 10^4 points drawn) and oa_stability (of the drawn points, and of the
whole cloud) beside oa_voxel_downsample of the same cloud, same build, same GPU, same run.

The cloud is a bumpy unit sphere with its (slightly tilted) radial normals -- every bucket of the cube map is occupied, which is
what the sort and the level search cost most on --, host arrays in, host arrays out: the copies are part of every call's
total_ms, as they are for a caller.  Each call is warmed once and timed `reps` times; the least
total_ms (host time of the call, ending in a device synchronisation) is reported.  The voxel edge is chosen so that the
downsample keeps about 10^4 rows as well.  Prints one JSON line.  No pass/fail bar: DESIGN.md 3.21 records the numbers.

    python tools/sample_cost.py [--sizes 100000,1000000] [--m 10000] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from object_alignment_amd.engine import IcpEngine           # noqa: E402


def cloud(n, seed=7):
    """n points on a bumpy unit sphere and their (radial, slightly tilted) unit normals."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    xyz = d * (1.0 + 0.05 * np.sin(7.0 * d[:, :1]) * np.cos(5.0 * d[:, 1:2]))
    nrm = d + 0.1 * rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return xyz.astype(np.float32), nrm.astype(np.float32)


def total_ms(out):
    return float(out["report"]["total_ms"]) if "report" in out else float(out["total_ms"])


def least_ms(call, reps):
    call()                                                      # warm: code objects, the allocation cache
    return min(total_ms(call()) for _ in range(reps))


def leg(e, n, m, reps):
    xyz, nrm = cloud(n)
    voxel = float(np.sqrt(4.0 * np.pi / m))                     # ~m occupied cells on a unit sphere
    drawn = e.normal_space_sample(nrm, m)
    down = e.voxel_downsample(xyz, voxel, normals=nrm)
    out = {"n": n, "m": m, "drawn": int(len(drawn["idx"])), "bins_occupied": int(drawn["report"]["bins_occupied"]),
           "level": int(drawn["report"]["level"]), "voxel": round(voxel, 5), "voxel_rows": int(down["report"]["n_voxels"])}
    out["normal_space_sample_ms"] = round(least_ms(lambda: e.normal_space_sample(nrm, m), reps), 3)
    out["voxel_downsample_ms"] = round(least_ms(lambda: e.voxel_downsample(xyz, voxel, normals=nrm), reps), 3)
    out["stability_of_sample_ms"] = round(least_ms(lambda: e.stability(xyz, nrm, idx=drawn["idx"]), reps), 3)
    out["stability_of_all_ms"] = round(least_ms(lambda: e.stability(xyz, nrm), reps), 3)
    st = e.stability(xyz, nrm, idx=drawn["idx"])
    out["sample_rank"], out["sample_cond"] = st["rank"], round(st["cond"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--m", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    res = {"reps": args.reps, "legs": []}
    with IcpEngine(args.device) as e:
        for n in (int(t) for t in args.sizes.split(",")):
            res["legs"].append(leg(e, n, args.m, args.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
