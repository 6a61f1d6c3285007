"""The owning handle of device memory (csrc/oa_devbuf.hpp), on the host: tests/c/devbuf_lifetime.cpp includes the very header the
library includes and stands a counting allocator behind it.  `= {}` on a group of handles releases every live block once and
returns every plain member to its default; a move leaves its source empty; alloc on a live handle releases first; destruction
after reset() releases nothing; inside a DevTeardown scope (oa_destroy, behind its one device synchronisation) every release is
settled, outside it none is.  Built with AddressSanitizer and UBSan as a stand-alone program.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "object_alignment_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "devbuf_lifetime.cpp")


def test_handles_release_each_block_once_and_settled_only_in_a_teardown(tmp_path):
    exe = str(tmp_path / "devbuf_lifetime")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", exe, SRC])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode == 0, p.stdout[-2000:]
    assert " 0 checks failed" in p.stdout and "FAILED" not in p.stdout, p.stdout[-2000:]
