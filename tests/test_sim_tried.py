"""The tried set of a constrained random walk (csrc/sim_tried.hpp: plain C++, included by k_simulate_constrained with its own function qualifiers) without
a GPU: tests/sim_tried_main.cpp compares it with a naive list-based reference, built here with AddressSanitizer and UBSan.  Checked there: the pick-th
untried position for every pick, the count, "all tried" and membership, before every marking, for 1, 63, 64, 65, 128, 255 and 256 positions in ascending,
descending and 40 random orders, and in every order for 1 .. 6 positions; the over-width test."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tried_set_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone tried-set test"
    exe = str(tmp_path / "sim_tried")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "vsr_tlaplus_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sim_tried_main.cpp")],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) == sum([1, 2, 6, 24, 120, 720]) + 7 * 42      # every order of 1 .. 6 positions + (2 + 40) orders of each boundary size


def test_the_header_is_plain_cpp_and_the_kernel_uses_it():
    csrc = os.path.join(ROOT, "vsr_tlaplus_amd", "csrc")
    header = open(os.path.join(csrc, "sim_tried.hpp")).read()
    assert "hip" not in header.split("#pragma once")[1].lower() and "__device__" not in header
    kernel = open(os.path.join(csrc, "vsr_sim_constrain.hpp")).read()
    assert '#include "sim_tried.hpp"' in kernel
    for fn in ("tried_pick(", "tried_mark(", "tried_all(", "tried_fits(", "tried_clear("):
        assert fn in kernel, fn
