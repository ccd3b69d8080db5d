"""What names the action of an instance ordinal (csrc/regen_ord.hpp: plain C++, included by k_regen_bits with its own function qualifiers) without a GPU:
tests/regen_ord_main.cpp gives every ordinal range to the helper and holds the result against the order in which the oracle's `successors` enumerates the
same instances, built here with AddressSanitizer and UBSan.  That the order written down there IS the oracle's is read from oracle/vsr_oracle.cpp."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ordinal_naming_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone ordinal test"
    exe = str(tmp_path / "regen_ord")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "vsr_tlaplus_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "regen_ord_main.cpp")],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok 12\n" and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]   # R = 2, 3 x C = 1, 2 x |Values| = 1 .. 3


def test_the_order_checked_is_the_oracles_and_the_kernel_uses_the_helper():
    src = open(os.path.join(ROOT, "oracle", "vsr_oracle.cpp")).read()
    body = src[src.index("  TimerSendSVC(P, s, out);"):]
    calls = re.findall(r"^  (\w+)\(P, s, out\);", body, re.M)[:15]
    replica_bound = [c for c in calls if c in ("TimerSendSVC", "SendDVC", "SendSV", "ReceiveClientRequest", "ExecuteOp")]
    assert replica_bound == ["TimerSendSVC", "SendDVC", "SendSV", "ReceiveClientRequest", "ExecuteOp"], calls    # the order regen_ord_main.cpp writes down
    rcr = src[src.index("static void ReceiveClientRequest("):]
    loops = re.findall(r"for \(int (\w) = 1; \w <= P\.(\w)", rcr[:400])
    assert [v for v, _ in loops[:2]] == ["r", "c"], loops                                                      # replica, then client (then value)
    csrc = os.path.join(ROOT, "vsr_tlaplus_amd", "csrc")
    header = open(os.path.join(csrc, "regen_ord.hpp")).read()
    assert "hip" not in header.split("#pragma once")[1].lower() and "__device__" not in header
    kernel = open(os.path.join(csrc, "vsr_regen_bits.hpp")).read()
    assert '#include "regen_ord.hpp"' in kernel and "regen_ord(M.R, M.C, M.n, ord)" in kernel
