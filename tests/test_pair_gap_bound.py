"""Level 0 of k_nn_search_sorted on pairs of vertices (csrc/oa_pairgap.hpp): the rounding bound its threshold rests on,

    pair_gap(m, w, h) <= (g + pair_allowance(qmax, h)) (1 + 2^-23),     g the real smaller gap of the pair,

checked against long double by a stand-alone host program (tests/c/pair_gap_bound.cpp) that includes the very header the kernel
and the upload include: >= 1e7 random triples and the adversarial ones -- a point on a vertex, on the pair's midpoint and an ulp
to either side of it, q1 == q2, pairs one ulp apart, scales 1e-30 .. 1e18, both padding rules.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "object_alignment_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "pair_gap_bound.cpp")


def test_pair_gap_never_overstates_the_real_gap_by_more_than_its_allowance(tmp_path):
    exe = str(tmp_path / "pair_gap_bound")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, SRC])
    p = subprocess.run([exe, "10000000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    assert "0 violations" in p.stdout and " 10000000 random" in p.stdout, p.stdout[-2000:]
