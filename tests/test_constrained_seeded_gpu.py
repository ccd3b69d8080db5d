"""The constrained level step on harvested states at FIVE and FOUR replicas and at TWO clients, GPU leg (`-m gpu`).

k_constrain, k_step_expand (a second successor writer beside k_expand, with its own room reservation and its own actc_write_child), k_step_keep and the gated trace
decide what a search contains.  test_constraint_gpu.py never leaves three replicas and one client; test_action_constraint_gpu.py meets five replicas and two clients
seven levels from Init under the constraint TRUE, where nothing is blocked, and compares counts and checksums.  No test of either file compares a RECORD
k_step_expand wrote with the oracle's: the kernel takes a state's fingerprint from the hashes of the Delta, not from the words it stored, so a wrong store — the
fourth word of a replica block at R >= 4, a patched bag word, the fourth appended entry of a broadcast, a view hash — would show only one level later.

Here the 1500-state sample (deep_predicates_reference.state_indices) of the harvest of (5,1,2,1), (4,1,2,1) and (3,2,3,1) is seeded as level 1 of a constrained
checker in a child process (tests/constrained_seeded_worker.py under libvsrmc_hooks.so; one child per space, one checker per case) and stepped once or twice under
constraints that read what exists only at R >= 4 or C = 2; every figure, every record of every level and a sample of traces are held against
tests/constrained_seeded_reference.py (the C++ CPU oracle and hand-written Python predicates).  The non-vacuity floors are test_constrained_seeded_cpu.py's."""
import json
import os
import subprocess
import sys

import pytest

import constrained_seeded_reference as cs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = {(5, 1, 2, 1): 600, (4, 1, 2, 1): 300, (3, 2, 3, 1): 300}      # per child, seconds (measured: README.md, the tests paragraph)


@pytest.mark.parametrize("key", cs.SPACES, ids=cs.IDS)
def test_constrained_steps_on_the_seeded_level(key, tmp_path):
    hooks = os.path.join(ROOT, "vsr_tlaplus_amd", "libvsrmc_hooks.so")
    assert os.path.exists(hooks), "build it: python vsr_tlaplus_amd/build.py"
    out = os.path.join(str(tmp_path), "constrained_seeded.json")
    env = {k: v for k, v in os.environ.items() if k not in ("VSRMC_ACTION_SLICE", "VSRMC_ACTION_LIST_CAP", "VSRMC_CONSTRAIN_GRID", "VSRMC_WHERE_LIST_CAP")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "constrained_seeded_worker.py")] + [str(x) for x in key] + [out],
                       capture_output=True, text=True, timeout=TIMEOUT[key], env=dict(env, VSRMC_LIB=hooks))
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    with open(out) as f:
        res = json.load(f)
    want = cs.MEASURED[key]
    assert res["seeds"] == 1500 and sorted(res["cases"]) == ["a", "b", "c", "d"] + (["e"] if key[1] == 2 else [])
    # what the worker compared is what the CPU leg floors: a run over another sample would not pass for this one
    c2, c3 = res["cases"]["c"]
    for lv, row in ((c2, want["level2"]), (c3, want["level3"])):
        assert lv["action"]["blocked"] >= (row["blocked"] + 1) // 2 and lv["state"]["pruned"] >= (row["pruned"] + 1) // 2
        assert lv["state"]["kept"] >= (row["kept"] + 1) // 2 and lv["traces"] >= 16
    assert [lv["level"] for lv in res["cases"]["c"]] == [2, 3]
    assert res["cases"]["a"][0]["action"]["blocked_violating"] >= (1 if want["viol_blocked"] else 0)
    assert (res["cases"]["d"][0]["viol"][1] != 0) == (want["viol_new_second"] > 0)
    assert res["scan"]["n_pairs"] == c2["action"]["permitted"]
    if key[0] == 5:
        assert sorted(res["regimes"]) == ["grid1", "listcap64", "slice64"] and sum(res["regimes"]["listcap64"]["relisted"]) > 0
    print("child of %s: %.1f s" % (key, res["seconds"]))
