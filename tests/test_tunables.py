"""csrc/oa_tunables.hpp: every OA_* knob is read once, into one struct.  A stand-alone program (tests/c/print_tunables.cpp: its own
main, nothing of the library but that header, no HIP) prints the struct under chosen environments, in both flavours.  The expected
values are those of the code the header replaced; "was" cites the line of oa_icp.hip at commit 74f9a8a that held the parse."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "object_alignment_amd", "csrc", "oa_tunables.hpp")


@pytest.fixture(scope="module")
def printers(tmp_path_factory):
    out = {}
    for flavour, flags in (("default", []), ("experiments", ["-DOA_EXPERIMENTS"])):
        exe = str(tmp_path_factory.mktemp("tunables") / ("print_tunables_" + flavour))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", os.path.dirname(HEADER),
                               os.path.join(ROOT, "tests", "c", "print_tunables.cpp"), "-o", exe])
        out[flavour] = exe
    return out


def _read(exe, env=None, *args):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("OA_")}
    clean.update(env or {})
    p = subprocess.run([exe] + list(args), env=clean, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    return dict(ln.split("=", 1) for ln in p.stdout.splitlines())


def _struct_fields():
    text = open(HEADER).read()
    body = text[text.index("struct Tunables {"):]
    body = body[:body.index("\n};")]
    return re.findall(r"^\s+(?:bool|int|double) (\w+) = ", body, re.M)


def test_header_is_plain_cxx():
    """no HIP header, only the three standard ones"""
    includes = re.findall(r"^#include\s+(\S+)", open(HEADER).read(), re.M)
    assert sorted(includes) == ["<algorithm>", "<cstdlib>", "<cstring>"]


def test_every_field_is_printed(printers):
    fields = _struct_fields()
    assert len(fields) > 70 and len(set(fields)) == len(fields)
    printed = [k for k in _read(printers["default"]) if not k.startswith("cache.")]
    assert printed == fields


@pytest.mark.parametrize("flavour", ["default", "experiments"])
def test_unset_environment_gives_the_initialisers(printers, flavour):
    got, dflt = _read(printers[flavour]), _read(printers[flavour], None, "defaults")
    assert got == dflt
    # ... and the initialisers are the defaults the call sites had (was: the line cited)
    was = {"nn_grid": "-1",                  # 2221
           "nn_r": "0",                      # 2186
           "grid_lanes": "0",                # 2189
           "grid_safe": "1",                 # 2195
           "nn_persist": "4",                # 2211
           "nn_queue_min": "-1",             # 2213
           "nn_mfma": "0",                   # 2214
           "list_blocks_per_cu": "16",       # 2204
           "tri_fine_min_tris": "200000",    # 2201
           "tree_acc_max": "4096",           # 2223
           "grid_path": "0",                 # 2226
           "acc_blocks": "512",              # 591
           "time_events": "-1",              # 1421: unset -> 1 for brute force, else 0
           "nn_target_blocks": str(-2 ** 31),  # 572: unset -> want_auto
           "grid_rmax": "3",                 # 2609, 2961
           "grid_budget": "256",             # 2613
           "tri_budget": "192",              # 2963
           "tri_max_cells_log2": "24",       # 2944
           "tri_xcd_chunk": "8",             # 2971
           "tri_drop_over": "1",             # 2969
           "tri_fine_cap": "192",            # 3072
           "multi_threads": "-1",            # 2288
           "exchange": "-1",                 # 1548: OA_EXCHANGE_AUTO
           "mailbox": "0",                   # 1849
           "fault_stall_iter": "2",          # 2277
           "debug": "0",                     # 2192
           "cache.enabled": "1", "cache.cap_given": "0"}   # 106, 107
    for k, v in was.items():
        assert got[k] == v, k
    reals = {"turn_frac": 0.1, "grid_ppc": 2.0, "grid_budget_moving": 2.0, "tri_budget_moving": 3.0, "tri_cell": 1.25,     # 2206, 2585, 2614, 2964, 2940
             "tri_moving_frac": 0.25, "tri_xcd_moving_frac": 0.5, "tri_ring_cap": 0.25, "tri_fine_cell": 0.5,              # 2970, 2972, 2197, 3032
             "tri_fine_rho": 0.3, "tri_fine_max_mb": 8192.0, "tri_fine_gate": 1e30, "exchange_timeout_s": 30.0,            # 3033, 3040, 3073, 2266
             "cache.cap_mb": 256.0}                                                                                        # 108
    for k, v in reals.items():
        assert float(got[k]) == v, k


# (environment, field, value in the default library, value with -DOA_EXPERIMENTS)
CASES = [
    ({"OA_GRID_SAFE": "7"}, "grid_safe", "2", "2"),                          # 2195: clamped to 0..2
    ({"OA_NN_R": "3"}, "nn_r", "0", "0"),                                    # 2187: not 1 / 2 / 4 / 8 -> auto
    ({"OA_NN_R": "8"}, "nn_r", "4", "8"),                                    # 2218: 8 is an experiments instantiation
    ({"OA_NN_MFMA": "1"}, "nn_mfma", "0", "1"),                              # 2214, 2217: inert in the default library
    ({"OA_NN_PERSIST": "99"}, "nn_persist", "16", "16"),                     # 2211
    ({"OA_LIST_BLOCKS_PER_CU": "0"}, "list_blocks_per_cu", "1", "1"),        # 2204
    ({"OA_TRI_FINE_MIN_TRIS": "1"}, "tri_fine_min_tris", "64", "64"),        # 2201
    ({"OA_TRI_MAX_CELLS_LOG2": "40"}, "tri_max_cells_log2", "29", "29"),     # 2944
    ({"OA_TRI_XCD_CHUNK": "-3"}, "tri_xcd_chunk", "0", "0"),                 # 2971
    ({"OA_GRID_BUDGET": "100000"}, "grid_budget", "100000", "100000"),       # 2613: the vertex grid's is not clamped
    ({"OA_GRID_BUDGET": "100000"}, "tri_budget", "30000", "30000"),          # 2963
    ({"OA_GRID_BUDGET_MOVING": "1"}, "grid_budget_moving", "1", "1"),        # 2614
    ({"OA_GRID_BUDGET_MOVING": "1"}, "tri_budget_moving", "1", "1"),         # 2964
    ({"OA_GRID_RMAX": "5"}, "grid_rmax", "3", "3"),                          # 2609, 2961
    ({"OA_GRID_PATH": "fast"}, "grid_path", "1", "1"),                       # 2226
    ({"OA_GRID_PATH": "safe"}, "grid_path", "2", "2"),
    ({"OA_GRID_PATH": "other"}, "grid_path", "0", "0"),
    ({"OA_EXCHANGE": "RCCL"}, "exchange", "1", "1"),                         # 2283: OA_EXCHANGE_RCCL
    ({"OA_EXCHANGE": "mailbox"}, "exchange", "0", "0"),                      # 2284: OA_EXCHANGE_MAILBOX
    ({"OA_EXCHANGE": "x"}, "exchange", "-1", "-1"),                          # neither: OA_EXCHANGE_AUTO stays
    ({"OA_EXCHANGE_TIMEOUT_S": "0"}, "exchange_timeout_s", "0.05", "0.05"),  # 2266
    ({"OA_MAILBOX": "host"}, "mailbox", "1", "1"),                           # 1850
    ({"OA_MAILBOX": "device"}, "mailbox", "2", "2"),
    ({"OA_MAILBOX": "Device"}, "mailbox", "0", "0"),
    ({"OA_GRID_LANES": ""}, "grid_lanes", "0", "0"),                         # 231: empty is unset
    ({"OA_GRID_LANES": "4"}, "grid_lanes", "4", "4"),                        # 2189
    ({"OA_DEBUG": ""}, "debug", "1", "1"),                                   # 2192: on when the variable exists
    ({"OA_TIME_EVENTS": "0"}, "time_events", "0", "0"),                      # 1421
    ({"OA_TIME_EVENTS": "5"}, "time_events", "1", "1"),
    ({"OA_NN_TARGET_BLOCKS": "640"}, "nn_target_blocks", "640", "640"),      # 572
    ({"OA_NN_SORT": "0"}, "nn_sort", "1", "0"),                              # 2208, 2217
    ({"OA_TRI_RING": "2"}, "tri_ring", "0", "2"),                            # 2196, 2217
    ({"OA_TRI_FINE": "9"}, "tri_fine", "0", "2"),                            # 2200, 2217
    ({"OA_GRID_STATS": "1"}, "grid_stats", "0", "1"),                        # 2193, 2217
    ({"OA_TRI_SHARE": "0"}, "tri_share", "1", "0"),                          # 2194, 2217
    ({"OA_TRI_FINE_RHO": "9"}, "tri_fine_rho", "4", "4"),                    # 3033
    ({"OA_DEV_CACHE": "0"}, "cache.enabled", "0", "0"),                      # 106
    ({"OA_DEV_CACHE": ""}, "cache.enabled", "0", "0"),                       # 106: off for whatever atoi reads as 0
    ({"OA_DEV_CACHE": "1"}, "cache.enabled", "1", "1"),
    ({"OA_DEV_CACHE_MB": "-4"}, "cache.cap_mb", "0", "0"),                   # 108
    ({"OA_DEV_CACHE_MB": "64"}, "cache.cap_given", "1", "1"),                # 107
    ({"OA_DEV_CACHE_MB": ""}, "cache.cap_given", "0", "0"),
]


@pytest.mark.parametrize("env,field,plain,exp", CASES, ids=["%s=%s->%s" % (*list(c[0].items())[0], c[1]) for c in CASES])
def test_parse_and_clamp(printers, env, field, plain, exp):
    for flavour, want in (("default", plain), ("experiments", exp)):
        got = _read(printers[flavour], env)[field]
        assert float(got) == float(want), (flavour, got)


def _csrc_files():
    d = os.path.dirname(HEADER)
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith((".hip", ".hpp", ".h", ".cpp"))]


def test_only_the_header_reads_the_environment():
    for path in _csrc_files():
        if path == HEADER:
            continue
        text = open(path).read()
        assert not re.search(r"\bgetenv\b|\benv_int\(|\benv_double\(", text), path


def test_design_table_lists_exactly_the_knobs_the_header_reads():
    """DESIGN 8 is the one table of the knobs: its names are the header's string literals, plus the rows marked as read by Python"""
    in_header = set(re.findall(r'"(OA_[A-Z0-9_]+)"', open(HEADER).read()))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("\n## 8. "):design.index("\n## 9. ")]
    rows = [ln for ln in section.splitlines() if ln.startswith("| `OA_")]
    native, python = set(), set()
    for row in rows:
        names = re.findall(r"`(OA_[A-Z0-9_]+)`", row.split("|")[1])
        assert len(names) == 1, row                             # full names, one per row
        (python if "read by Python" in row else native).add(names[0])
    assert len(in_header) > 70
    assert native == in_header, (sorted(native - in_header), sorted(in_header - native))
    assert python == {"OA_DEVICES", "OA_ICP_LIB", "OA_ICP_LIB_DEBUG"}
