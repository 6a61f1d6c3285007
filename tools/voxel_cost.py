"""What a voxel downsample costs: oa_voxel_downsample on n points of the synthetic bunny -- a sparse pass over the
whole surface plus a dense pass over a cap, so that the rows' lengths are skewed -- at three voxel sizes, from host memory and from
a device tensor, beside the same result from numpy on the host (np.unique over the keys, np.add.at for the sums; no
representative, which numpy has no one-pass way to).

One GPU process.  Times are host clocks around calls that end in a device synchronise, best of --reps after a warm-up; the
library's own report (total_ms of the call) is printed next to them.  Prints one JSON line.  No pass/fail bar.

    python tools/voxel_cost.py [--n 1000000] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inputs(n):
    from object_alignment_amd import synth
    sparse, ns = synth.bunny_surface_with_normals(n // 2, 0.37)
    dense, nd = synth.bunny_surface_with_normals(2 * n + 64, 0.11)
    cap = np.flatnonzero(dense[:, 2] > 0.5 * np.linalg.norm(dense, axis=1))[: n - len(sparse)]
    xyz, nrm = np.concatenate([sparse, dense[cap]]), np.concatenate([ns, nd[cap]])
    order = np.random.default_rng(7).permutation(len(xyz))
    return np.ascontiguousarray(xyz[order]), np.ascontiguousarray(nrm[order])


def best_ms(f, reps):
    f()                                       # warm-up: code objects, the allocation cache
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return best


def numpy_downsample(xyz, nrm, voxel):
    p = xyz.astype(np.float64)
    o = p.min(axis=0)
    c = np.floor((p - o) / voxel).astype(np.int64)
    d = c.max(axis=0) + 1
    key = (c[:, 2] * d[1] + c[:, 1]) * d[0] + c[:, 0]
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    mean = np.zeros((len(cnt), 3))
    nsum = np.zeros((len(cnt), 3))
    np.add.at(mean, inv, p)
    np.add.at(nsum, inv, nrm.astype(np.float64))
    mean /= cnt[:, None]
    nsum /= np.maximum(1e-300, np.linalg.norm(nsum, axis=1, keepdims=True))
    return mean.astype(np.float32), nsum.astype(np.float32), cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--voxels", type=float, nargs="+", default=[0.01, 0.03, 0.1])
    args = ap.parse_args()
    import torch
    from object_alignment_amd.engine import IcpEngine
    xyz, nrm = inputs(args.n)
    res = {"n": len(xyz), "reps": args.reps, "voxels": []}
    with IcpEngine(args.device) as e:
        dx, dn = torch.from_numpy(xyz).cuda(args.device), torch.from_numpy(nrm).cuda(args.device)
        for h in args.voxels:
            got = []
            row = {"voxel": h}
            row["host_arrays_ms"] = best_ms(lambda: got.append(e.voxel_downsample(xyz, h, normals=nrm)), args.reps)
            row["device_tensors_ms"] = best_ms(lambda: got.append(e.voxel_downsample(dx, h, normals=dn)), args.reps)
            row["device_tensors_no_normals_ms"] = best_ms(lambda: got.append(e.voxel_downsample(dx, h)), args.reps)
            rep = got[-1]["report"]
            row.update(n_voxels=rep["n_voxels"], max_members=rep["max_members"], dims=list(rep["dims"]), library_total_ms=rep["total_ms"])
            ref = []
            row["numpy_unique_ms"] = best_ms(lambda: ref.append(numpy_downsample(xyz, nrm, h)), max(1, min(args.reps, 2)))
            row["numpy_rows"] = int(len(ref[-1][2]))
            row["largest_mean_difference"] = float(np.abs(got[0]["xyz"].astype(np.float64) - ref[-1][0]).max()) if len(ref[-1][2]) == rep["n_voxels"] else None
            res["voxels"].append(row)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
