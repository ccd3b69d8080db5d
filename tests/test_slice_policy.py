"""The slice policy of the k_step_list driver (csrc/host_slice_policy.hpp: plain host C++, no HIP) without a GPU: tests/slice_policy_main.cpp drives it with
a scripted number of instances per parent in the place of the kernel, built here with AddressSanitizer and UBSan.  Checked there: every parent index lies
in exactly one accepted slice, no accepted slice had more instances than the list holds, a single parent above the capacity ends with the failure; 1, 63,
64, 65 and 1000 parents, a list of 64 entries, instances all zero, all one, one spike of 65, a dense run in the middle; the first slice, the halving, the
growing back and the adaptive rule number by number."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slice_policy_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone policy test"
    exe = str(tmp_path / "slice_policy")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "vsr_tlaplus_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "slice_policy_main.cpp")],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) == 5 * 4 * 4 * 3                  # shapes x patterns x first sizes x policies


def test_the_driver_uses_this_policy_and_nothing_else():
    """the three former copies of the loop are gone: k_step_list is launched in one place, and the policy header has no HIP in it"""
    csrc = os.path.join(ROOT, "vsr_tlaplus_amd", "csrc")
    picks = [f for f in sorted(os.listdir(csrc)) if "k_step_list<" in open(os.path.join(csrc, f)).read() or "(k_step_list" in open(os.path.join(csrc, f)).read()]
    assert picks == ["host_step_slices.hpp"], picks                  # (vsr_step.hpp defines the template: `k_step_list(Model M, ...`)
    policy = open(os.path.join(csrc, "host_slice_policy.hpp")).read()
    assert "hip" not in policy.split("#pragma once")[1].lower()
