"""The primitives every index build on the device goes through, each against numpy, exactly: the one-workgroup bitonic sort
and the LSD argsort of oa_sort.hpp (stable: equal keys stay in index order -- that fixes the slot order and the tree leaves, and
with them the order of every fp64 sum), the three-launch scan_counts_ll, the one-workgroup k_scan_counts behind make_pairs'
compaction, k_gather_int, and the compaction itself end to end through IcpEngine.make_pairs.

tools/sort_check.exe (built by __graft_entry__.build_tools()) holds no reference: it reads inputs from files, runs the library's
code and writes the device's output; it also keeps guard zones round every output and round a temporary buffer of exactly
sort_order_tmp_bytes(n) / scan_tmp_bytes(n) bytes, and reads the inputs back.  The references are here:
np.argsort(keys & mask, kind="stable"), np.lexsort for the orders by several keys (lex_order_next), np.cumsum in int64, src[idx].  One process per test, many cases each."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1
DIGIT_BITS, TILE = 10, 2048                      # oa_sort.hpp: SORT_BITS, SORT_TILE (= SCAN_TILE)


def sort_check_exe():
    import __graft_entry__ as entry
    exe = [e for e in entry.build_tools() if e.endswith("sort_check.exe")]
    assert exe, "tools/sort_check.hip did not build"
    assert os.path.exists(exe[0])
    return exe[0]


# ---------------------------------------------------------------------------------------------------------------------
# the cases of one process: (name, manifest words before the files, input arrays, expected output)
# ---------------------------------------------------------------------------------------------------------------------
def mask_of(bits):
    return np.uint32((1 << bits) - 1)


def sort_case(name, mode, bits, keys):
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    assert np.array_equal(keys & mask_of(bits), keys), name     # (the sorts' contract: the bits above `bits` are zero)
    want = np.argsort(keys & mask_of(bits), kind="stable").astype(np.int32)
    return ("sort %s bits=%d n=%d %s" % (mode, bits, len(keys), name), ["sort", mode, str(bits), str(len(keys))], [keys], want)


def lex_case(name, bits, keys):
    """keys: the least significant key first, as np.lexsort takes them (its last key is the primary one)"""
    keys = [np.ascontiguousarray(k, dtype=np.uint32) for k in keys]
    for b, k in zip(bits, keys):
        assert np.array_equal(k & mask_of(b), k), name
    want = np.lexsort(keys).astype(np.int32)
    return ("lex bits=%s n=%d %s" % (bits, len(keys[0]), name), ["lex", str(len(keys)), str(len(keys[0]))] + [str(b) for b in bits], keys, want)


def scan_case(name, mode, counts):
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    want = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)
    return ("scan %s n=%d %s" % (mode, len(counts), name), ["scan", mode, str(len(counts))], [counts], want)


def gather_case(name, src, idx):
    src, idx = np.ascontiguousarray(src, dtype=np.int32), np.ascontiguousarray(idx, dtype=np.int32)
    return ("gather n_src=%d n=%d %s" % (len(src), len(idx), name), ["gather", str(len(src)), str(len(idx))], [src, idx], src[idx])


def run_cases(tmp_path, cases):
    """One sort_check process over all the cases; every output compared exactly.  A non-zero exit (a HIP error, a violated guard,
    a changed input) fails at once with the tool's output; wrong results are collected and named together."""
    exe = sort_check_exe()
    lines, outs = [], []
    for k, (name, words, inputs, want) in enumerate(cases):
        files = []
        for j, a in enumerate(inputs):
            path = os.path.join(str(tmp_path), "c%d_in%d.bin" % (k, j))
            a.tofile(path)
            files.append(path)
        outs.append(os.path.join(str(tmp_path), "c%d_out.bin" % k))
        lines.append(" ".join(words + files + [outs[-1]]))
    manifest = os.path.join(str(tmp_path), "manifest.txt")
    with open(manifest, "w") as f:
        f.write("\n".join(lines) + "\n")
    p = subprocess.run([exe, manifest], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:]
    verdicts = [ln for ln in p.stdout.splitlines() if ln.startswith("case ")]
    assert len(verdicts) == len(cases) and ("%d cases done" % len(cases)) in p.stdout, p.stdout[-3000:]
    for ln in verdicts:
        assert ln.endswith("guards ok inputs untouched"), ln
    wrong = []
    for (name, _, _, want), path in zip(cases, outs):
        got = np.fromfile(path, dtype=want.dtype)
        if got.shape != want.shape:
            wrong.append("%s: %d elements, not %d" % (name, got.size, want.size))
        elif not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            wrong.append("%s: %d of %d differ, first at %d (%d, not %d)" % (name, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]]))
        os.unlink(path)
    for f in os.listdir(str(tmp_path)):
        if f.endswith(".bin"):
            os.unlink(os.path.join(str(tmp_path), f))
    assert not wrong, "\n".join(wrong)


# ---------------------------------------------------------------------------------------------------------------------
# key patterns (all within the low `bits` bits)
# ---------------------------------------------------------------------------------------------------------------------
def keys_ties(n, bits, seed):
    """tools/sort_bench.hip's pattern: random keys, every fifth one a copy of k[i / 2]"""
    k = np.random.default_rng(seed).integers(0, 1 << bits, size=n, dtype=np.uint64).astype(np.uint32)
    for i in range(0, n, 5):
        k[i] = k[i // 2]
    return k


def keys_few(n, bits, seed, distinct=7):
    """many ties: `distinct` values spread over the key range"""
    rng = np.random.default_rng(seed)
    values = rng.integers(0, 1 << bits, size=distinct, dtype=np.uint64).astype(np.uint32)
    return values[rng.integers(0, distinct, size=n)]


def keys_from_digits(digits, bits):
    """digits[p][i] = the digit of item i in pass p"""
    k = np.zeros(len(digits[0]), np.uint64)
    for p, d in enumerate(digits):
        k |= np.asarray(d, np.uint64) << np.uint64(DIGIT_BITS * p)
    return (k & np.uint64((1 << bits) - 1)).astype(np.uint32)


def lsd_patterns(n, bits, seed):
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    passes = (bits + DIGIT_BITS - 1) // DIGIT_BITS
    top = 1 << bits
    out = [("ties", keys_ties(n, bits, seed)),
           ("all equal", np.full(n, 0x2AAAAAAA & (top - 1), np.uint32)),                 # one bin takes every item, in every pass
           ("two values", np.where(i % 2 == 0, (top - 1) & 0x3FF003FF, 0x00000C01 & (top - 1)).astype(np.uint32)),
           ("ascending", i.astype(np.uint32)),
           ("descending", (n - 1 - i).astype(np.uint32)),
           ("digit = i mod 1024", keys_from_digits([i % 1024] * passes, bits)),      # every lane of a round its own peer group
           ("digit constant per round of 64", keys_from_digits([((i // 64) * m) % 1024 for m in (1, 341, 683, 5)[:passes]], bits)),
           ("digits 0 and 1023", keys_from_digits([1023 * rng.integers(0, 2, size=n) for _ in range(passes)], bits)),
           ("low 20 bits constant", ((rng.integers(0, 1024, size=n).astype(np.uint32) << np.uint32(20)) | np.uint32(0x5A5A5)) & np.uint32(top - 1)),
           ("high 20 bits constant", (np.uint32(0x2F0F3 << 10) | rng.integers(0, 1024, size=n).astype(np.uint32)) & np.uint32(top - 1))]
    if n % 64:
        k = keys_ties(n, bits, seed + 1)
        k[(n // 64) * 64:] = 0                                   # digit 0 in the last, partial round: beside the empty lanes' key 0
        k[rng.integers(0, n, size=max(1, n // 16))] = 0         # ... and more zeros before them
        out.append(("zeros in the ragged round", k))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# k_sort_small: sort_order up to 8192 keys
# ---------------------------------------------------------------------------------------------------------------------
def test_one_workgroup_sort_is_numpys_stable_argsort(tmp_path):
    """k_sort_small through oa::sort_order, around the padded power of two and the 1024-thread strides: random keys with many
    ties (bits 1, 30, 32), all keys equal (the index alone decides), strictly descending, and 32-bit keys with 0xFFFFFFFF
    among them (the composite key << 32 | i must sort in front of the ~0 padding)."""
    cases = []
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, 8191, 8192):
        i = np.arange(n, dtype=np.int64)
        cases.append(sort_case("one bit", "auto", 1, np.random.default_rng(n).integers(0, 2, size=n)))
        cases.append(sort_case("few values", "auto", 30, keys_few(n, 30, n + 1)))
        cases.append(sort_case("ties", "auto", 32, keys_ties(n, 32, n + 2)))
        cases.append(sort_case("all equal", "auto", 30, np.full(n, 123456, np.uint32)))
        cases.append(sort_case("descending", "auto", 30, (n - 1 - i) * 3))
    for n in (4097, 8191):
        k = keys_few(n, 32, n + 3)
        k[np.random.default_rng(n).integers(0, n, size=n // 3)] = 0xFFFFFFFF
        k[-1] = 0xFFFFFFFF
        cases.append(sort_case("with 0xFFFFFFFF", "auto", 32, k))
    run_cases(tmp_path, cases)


# ---------------------------------------------------------------------------------------------------------------------
# the LSD passes
# ---------------------------------------------------------------------------------------------------------------------
def test_lsd_sort_at_every_pass_count(tmp_path):
    """bits 1 ... 32 are 1, 1, 2, 2, 3, 3, 4, 4 passes: all four k_sort_scatter<PACKED_IN, LAST>, both k_sort_hist, the
    two-bit last digit -- with the kernels forced on one tile and a bit, and on 8193 keys."""
    cases = []
    for n in (2049, 8193):
        for bits in (1, 10, 11, 20, 21, 30, 31, 32):
            cases.append(sort_case("ties", "lsd", bits, keys_ties(n, bits, 100 * bits + n)))
            cases.append(sort_case("few values", "lsd", bits, keys_few(n, bits, 100 * bits + n + 1)))
    run_cases(tmp_path, cases)


def test_lsd_sort_at_ragged_sizes_and_chunk_edges(tmp_path):
    """30-bit keys: ragged rounds of 64, wave quarters of 512 and tiles of 2048 (the passes forced below 8193 keys, sort_order's
    own dispatch above); 256 tiles fill one chunk of k_sort_scan exactly, the 257th needs its carry; 32 bits at 257 tiles."""
    cases = []
    for n in (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049):
        cases.append(sort_case("ties", "lsd", 30, keys_ties(n, 30, n)))
    for n in (8193, 256 * TILE, 256 * TILE + 1, 1050001):
        cases.append(sort_case("ties", "auto", 30, keys_ties(n, 30, n)))
    cases.append(sort_case("ties", "auto", 32, keys_ties(256 * TILE + 1, 32, 32)))
    cases.append(sort_case("few values", "auto", 32, keys_few(256 * TILE + 1, 32, 33)))
    run_cases(tmp_path, cases)


@pytest.mark.parametrize("n", [2021, 2049, 8193, 8299, 256 * TILE + 1])
def test_lsd_sort_keeps_index_order_in_every_key_pattern(tmp_path, n):
    """Three passes over patterns that put all items in one bin, all lanes of a round in one peer group or each in its own,
    and passes that are no-ops on the keys and must keep the order the others made."""
    run_cases(tmp_path, [sort_case(name, "lsd", 30, k) for name, k in lsd_patterns(n, 30, n)])


# ---------------------------------------------------------------------------------------------------------------------
# orders by several keys: sort_order, then lex_order_next per further key
# ---------------------------------------------------------------------------------------------------------------------
LEX_WIDTHS = ((1, 1), (10, 11, 30), (32, 5), (3, 3, 3))              # the least significant key first
LEX_FEW = {(1, 1): (0, 1), (10, 11, 30): (0,), (32, 5): (1,), (3, 3, 3): (1,)}   # the keys that draw from fewer than 8 values


def test_lex_order_is_numpys_lexsort(tmp_path):
    """The edge sort of the normal orientation (w, lo, hi), the sampling's (bin, hash) and the voxel keys' slices all go through
    this: against np.lexsort, exactly, on either side of SORT_SMALL_MAX = 8192 (the only size at which the path switches), with
    two and three keys of widths from 1 to 32 bits, at least one key of every tuple drawing from fewer than 8 values (a one-bit key
    has two), and with all keys equal: then the order is the identity."""
    cases = []
    for n in (1, 2, 63, 8191, 8192, 8193, 20000):
        for widths in LEX_WIDTHS:
            keys = [keys_few(n, b, 1000 * n + 10 * j + b, distinct=min(5, 1 << b)) if j in LEX_FEW[widths] else keys_ties(n, b, 1000 * n + 10 * j + b)
                    for j, b in enumerate(widths)]
            assert all(len(np.unique(keys[j])) < 8 for j in LEX_FEW[widths])
            cases.append(lex_case("ties", widths, keys))
    for n in (8192, 20000):
        cases.append(lex_case("all equal", (10, 11, 30), [np.full(n, v, np.uint32) for v in (1023, 5, 0x2AAAAAAA)]))
        assert np.array_equal(cases[-1][3], np.arange(n, dtype=np.int32))
    run_cases(tmp_path, cases)


# ---------------------------------------------------------------------------------------------------------------------
# the scans
# ---------------------------------------------------------------------------------------------------------------------
def count_classes(n, seed, with_2_30):
    rng = np.random.default_rng(seed)
    some_max = rng.integers(0, 4, size=n).astype(np.int32)
    if n:
        some_max[rng.integers(0, n, size=min(n, 5))] = INT_MAX
        some_max[-1] = INT_MAX
    out = [("all zero", np.zeros(n, np.int32)), ("all one", np.ones(n, np.int32)),
           ("random 0..3", rng.integers(0, 4, size=n).astype(np.int32)), ("a few INT_MAX", some_max)]
    if with_2_30:
        out.append(("all 2^30", np.full(n, 1 << 30, np.int32)))     # the sums pass 2^31 and 2^32: a 32-bit accumulator anywhere shows
    return out


def test_scan_counts_ll_small_sizes(tmp_path):
    """scan_counts_ll round one item per thread (8), round a tile (2048) and on nothing (n = 0: the memset path)."""
    cases = []
    for n in (0, 1, 7, 8, 9, 2047, 2048, 2049):
        cases += [scan_case(name, "ll", c) for name, c in count_classes(n, n, with_2_30=n in (9, 2049))]
    run_cases(tmp_path, cases)


@pytest.mark.parametrize("n", [1024 * TILE, 1024 * TILE + 1])
def test_scan_counts_ll_second_round_of_tile_bases(tmp_path, n):
    """1024 tiles are one round of k_scan_tile_bases' 1024 threads, the 1025th tile takes the carry of the first round."""
    run_cases(tmp_path, [scan_case(name, "ll", c) for name, c in count_classes(n, n, with_2_30=False)])


def test_one_workgroup_scan_of_the_compaction(tmp_path):
    """k_scan_counts as oa_make_pairs launches it (one workgroup of 1024): ragged waves, one round exactly, the carry into a
    second and a third round."""
    cases = []
    for n in (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 3000):
        cases += [scan_case(name, "block", c) for name, c in count_classes(n, 7 * n + 1, with_2_30=True)]
    run_cases(tmp_path, cases)


# ---------------------------------------------------------------------------------------------------------------------
# the gather
# ---------------------------------------------------------------------------------------------------------------------
def test_gather_int(tmp_path):
    """k_gather_int with sort_ints' launch shape (blocks of 256): a permutation, and indices with repeats into a shorter src."""
    cases = []
    for n in (1, 255, 256, 257, 100000):
        rng = np.random.default_rng(n)
        src = rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)
        cases.append(gather_case("permutation", src, rng.permutation(n)))
        n_src = max(1, n // 3)
        cases.append(gather_case("repeats", src[:n_src], rng.integers(0, n_src, size=n)))
    run_cases(tmp_path, cases)


# ---------------------------------------------------------------------------------------------------------------------
# the ordered compaction end to end: k_block_counts, k_scan_counts, k_scatter_pairs behind make_pairs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [262144, 262145, 600001])
def test_make_pairs_compaction_keeps_selection_order(n):
    """The target is a cloud, the source the same cloud with a chosen subset moved 8 away in x: a moved point is further than
    thresh from everything, an unmoved one finds itself (or a bitwise-equal twin) at distance 0.  So A is the unmoved points
    in selection order and B the same bits.  1024 blocks of 256 are one round of k_scan_counts, 1025 carry into a single
    block, 600001 points are three rounds."""
    from object_alignment_amd.engine import IcpEngine
    rng = np.random.default_rng(n)
    pts = rng.random((n, 3), dtype=np.float32)
    i = np.arange(n)
    half = rng.random(n) < 0.5
    blocks = (i // 256) % 2 == 1
    blocks[(n - 1) // 256 * 256:] = False                        # the last block, ragged or not, stays
    ends = np.ones(n, bool)
    ends[[0, n - 1]] = False
    runs = [("random half", half, None), ("alternate blocks", blocks, None), ("all but the two ends", ends, None),
            ("nothing", np.zeros(n, bool), None)]
    if n == 262145:
        runs.append(("random half, vlist descending", half, i[::-1].copy()))
    eye = np.identity(4, dtype=np.float32)
    with IcpEngine(0) as eng:
        eng.set_search_mode("auto")
        eng.set_target(pts)
        for name, moved, vlist in runs:
            src = pts.copy()
            src[moved, 0] += np.float32(8.0)
            eng.set_source(src, vlist=vlist, stride=1)
            eng.set_matrices(eye, eye)
            A, B, _ = eng.make_pairs(0.25)
            order = i if vlist is None else vlist
            want = np.ascontiguousarray(src[order[~moved[order]]].T.astype(np.float64))
            assert A.shape == want.shape, (name, A.shape, want.shape)
            assert A.tobytes() == want.tobytes(), (name, "first wrong column", int(np.flatnonzero((A != want).any(axis=0))[0]))
            assert B.tobytes() == A.tobytes(), name
