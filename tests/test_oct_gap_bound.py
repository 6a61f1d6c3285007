"""Level 0 of k_nn_search_sorted on quads of vertices and pairs of points (csrc/oa_octgap.hpp): the rounding bound its threshold
rests on,

    oct_gap(mm, ww, ws, hm, hw') <= (T + oct_allowance(qmax, h1, h2, c) + e) (1 + 2^-23),     T the smallest real gap of the eight pairs,

and quad_threshold >= (max(sqrt(base_a), sqrt(base_b)) + allowance + e)(1 + 2^-22), checked against long double by a stand-alone host
program (tests/c/oct_gap_bound.cpp) that includes the very header the upload, the set-up and the kernel include: >= 1e7 random
octuples and the adversarial ones -- Hw < c, Hw = c, Hw = 0; WW > c, WW = c, WW = 0; pair widths orders of magnitude apart;
|X| = hw' and ||X| - hw'| = WW' and an ulp to either side of each; a point on a vertex with everything else far away; scales
1e-30 .. 1e18; offsets of 1e4 with spacing 1e-3; c = 0 and c huge; every padding rule.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "object_alignment_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "oct_gap_bound.cpp")


def test_oct_gap_never_overstates_the_smallest_real_gap_by_more_than_its_allowance_and_the_cap(tmp_path):
    exe = str(tmp_path / "oct_gap_bound")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, SRC])
    p = subprocess.run([exe, "10000000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    assert "0 violations" in p.stdout and " 10000000 random" in p.stdout, p.stdout[-2000:]
