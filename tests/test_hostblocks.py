"""csrc/pfc_hostblocks.h, the one statement of the blocks the host-pointer entry points move (value, seed, result, partial,
and the one-sync route's composed blocks): tests/hostblocks_check.cpp states the layouts a second time, with every offset
written out, and packs, compares and unpacks blocks at n = 1 and 3 items, 1 and 16 directions, ids / s / d_s given and not.
Built as a stand-alone program by the host compiler with AddressSanitizer and UBSan (every block is allocated to the byte, so a
wrong offset or size is a report) and run; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pressurefieldcontact.jl_amd", "csrc")


def test_hostblocks_layouts_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ or clang++) to build tests/hostblocks_check.cpp")
    exe = str(tmp_path / "hostblocks_check")
    # (g++: the sanitizer runtimes linked into the program, so that their place in the library order does not depend on the environment)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", *static, "-I", CSRC, os.path.join(ROOT, "tests", "hostblocks_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "hostblocks ok" in run.stdout, run.stdout + run.stderr
