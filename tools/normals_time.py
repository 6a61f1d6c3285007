"""Time oa_estimate_target_normals(k) beside the target upload (which builds the box tree) on bunny_surface clouds.

Wall time of the synchronous C calls on a warm context (the call waits for its stream), install = 1 and no host outputs, so that
no copy to the host is inside; the first call of each size is discarded, the rest give min / median.  One JSON line per size.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from object_alignment_amd import synth                     # noqa: E402
from object_alignment_amd.engine import IcpEngine          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    with IcpEngine(0) as e:
        for n in a.sizes:
            pts = synth.bunny_surface(n)
            up, est = [], []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                e.set_target(pts)
                t1 = time.perf_counter()
                e._chk(e._L.oa_estimate_target_normals(e._h, a.k, 2, None, 1, None, None))
                t2 = time.perf_counter()
                up.append(1e3 * (t1 - t0))
                est.append(1e3 * (t2 - t1))
            up, est = up[1:], est[1:]
            print(json.dumps(dict(n=n, k=a.k, reps=a.reps, set_target_ms_min=min(up), set_target_ms_median=statistics.median(up),
                                  estimate_ms_min=min(est), estimate_ms_median=statistics.median(est))), flush=True)


if __name__ == "__main__":
    main()
