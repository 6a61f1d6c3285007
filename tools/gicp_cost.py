"""What a GICP loop costs per iteration against a plane loop: same build, same GPU, same inputs.

Both metrics run search -> accumulate -> reduce + solve; the search, the reduction and the solve are the same launches.  The GICP
accumulation reads 12 B of source normal per slot more than the plane kernel and spends about 150 fp64 operations and one
division more per pair.  One leg, timed as loop_ms / iters_done of a loop that cannot end early:
  1M bunny points (analytic normals) on the 1.96M-triangle lattice mesh (bench.py's surface leg)
Prints one JSON line with plane_ms_per_iteration, gicp_ms_per_iteration and gicp_over_plane.  No pass/fail bar.

    python tools/gicp_cost.py [--n 1000000] [--steps 30]
"""
import argparse
import json
import os
import sys

import numpy as np

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--epsilon", type=float, default=1e-3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    verts, tris = synth.lattice_surface_mesh(700, 1400) if args.n >= 1_000_000 else synth.cubed_surface_mesh(40)
    pts, normals = synth.bunny_surface_with_normals(args.n, offset=0.37)
    mxa = synth.rigid4(synth.rotation_from_rotvec([0.02, -0.015, 0.025]), [0.01, -0.008, 0.012])
    mxb = np.identity(4, dtype=np.float32)
    res = {"n": args.n, "steps": args.steps, "n_tris": int(len(tris)), "gicp_epsilon": args.epsilon}
    with IcpEngine(args.device) as e:
        e.set_target_mesh(verts, tris)
        e.set_source(pts, stride=1)
        e.set_source_normals(normals)
        e.set_gicp(args.epsilon)
        for metric in ("plane", "gicp"):
            e.set_metric(metric)
            ms, r = per_iteration_ms(e, args.steps, 1, mxa, mxb)
            res[metric + "_ms_per_iteration"] = round(ms, 4)
            res[metric + "_last_K"] = r.last_K
    res["gicp_over_plane"] = round(res["gicp_ms_per_iteration"] / res["plane_ms_per_iteration"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
