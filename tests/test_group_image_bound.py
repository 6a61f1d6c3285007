"""Level 0 of k_nn_search_sorted on images of V = 8 and 16 sorted positions (group_image<V>, csrc/oa_octgap.hpp): the covering
property (P) on the stored floats -- 0 <= ww <= c, every real q_j within ws of mm + ww or of mm - ww -- and the bound the threshold
rests on,

    oct_gap(group_image, point_pair_image_capped) <= (T + oct_allowance(qmax, h1, h2, c) + e) (1 + 2^-23),   T the smallest of the 2V gaps,

checked against long double by a stand-alone host program (tests/c/group_image_bound.cpp) that includes the very header the upload,
the set-up and the kernel include: >= 1e7 random groups per V and the adversarial ones -- one outlier in a tight group; duplicates
(ww = ws = 0); halves further apart than 2 c, exactly 2 c and 0; c = 0 and c huge; Hw <, =, > c; scales 1e-30 .. 1e18; offsets of
1e4 with spacing 1e-3; every padding count 0 .. V, one vertex + V - 1 padding and V / 2 + V / 2 among them.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "object_alignment_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "group_image_bound.cpp")


def test_group_images_cover_their_vertices_and_never_overstate_the_smallest_gap(tmp_path):
    exe = str(tmp_path / "group_image_bound")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, SRC])
    p = subprocess.run([exe, "10000000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:]
    for v in (8, 16):
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("group_image_bound V=%d:" % v)]
        assert line and "0 violations" in line[0] and " 10000000 random" in line[0], p.stdout[-2000:]
