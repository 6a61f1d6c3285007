"""Level 0 of k_nn_search_sorted on pairs of vertices and pairs of points (csrc/oa_quadgap.hpp): the rounding bound its threshold
rests on,

    quad_gap(m, w, hm, hw) <= (T + quad_allowance(qmax, h1, h2)) (1 + 2^-23),     T the smallest real gap of the four pairs,

and quad_threshold >= (max(sqrt(base_a), sqrt(base_b)) + allowance)(1 + 2^-22), checked against long double by a stand-alone host
program (tests/c/quad_gap_bound.cpp) that includes the very header the kernel and the set-up include: >= 1e7 random quadruples and
the adversarial ones -- Hw < W, Hw = W, Hw = 0, W = 0, x = 0, |x| = Hw and an ulp to either side, a point on a vertex with its
partner far away, scales 1e-30 .. 1e18, offsets of 1e4 with spacing 1e-3, both padding rules.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "object_alignment_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "quad_gap_bound.cpp")


def test_quad_gap_never_overstates_the_smallest_real_gap_by_more_than_its_allowance(tmp_path):
    exe = str(tmp_path / "quad_gap_bound")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, SRC])
    p = subprocess.run([exe, "10000000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    assert "0 violations" in p.stdout and " 10000000 random" in p.stdout, p.stdout[-2000:]
