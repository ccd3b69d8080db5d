"""check_invariants_child of the two analysis models (csrc/vrst_actions.hpp, csrc/vras_actions.hpp) on VIOLATING states, on the GPU.

The invariants of VR_STATE_TRANSFER / VR_APP_STATE hold in every reachable state, so every other test compares the `inv` word of
k_successors with the oracle's on "0 == 0".  Here the parents are the mutants of tests/invariant_mutants.py (reachable states with the
replica variables edited inside the representation; classes A-F and the naive ones): for every parent the successor multiset
(action, fingerprint, auxkey, normalised record) of Model.second_model / third_model through the C ABI equals the C++ oracle's, and
for every child the `inv` word equals the oracle's verdict on that child's record under the cfg mask (14 / 30), under all bits
(15 / 31) and under every single bit.  The oracle evaluates every invariant alone; where its evaluation raises (an entry outside a
log: TLC's evaluation error) the kernels report the bit as violated, the rule their comment documents — including the case only the
pair r1 = r2 reads, a single replica with commit > Len(log).

Floors (tests/invariant_mutants.py check_floors, counted on the oracle's side and printed): per model and bit >= 200 children with the
bit set and >= 200 with it clear beside another violated bit of the parent, >= 5 per (bit, raised / cured by the step) that occurs at
all, every ordered pair (r1, r2) and position k <= n among the violating children of classes B and C, <= 1 % of the parents refused
by the oracle's `successors`.  Never produced by the generator (invariant_mutants.NEVER): bit 1 raised by a step (both models), bit 8
raised by a step of the second model.

The reporting path (k_expand's verdicts into viol_mask / viol_fp / trace, the probe's violator list) runs in a child process on a
seeded level: tests/model_seeded_worker.py."""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import invariant_mutants as im

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(model, space) for model in (2, 3) for space in im.SPACES]


@pytest.fixture(scope="module")
def vt():
    import vsr_tlaplus_amd as vt
    assert vt.load().vsrmc_device_count() >= 1, "no HIP device visible"
    return vt


def _expected(verdicts, mask):
    """the kernels' word under `mask`: every invariant of the mask that is violated or whose evaluation raises"""
    return sum(b for b, v in verdicts.items() if (mask & b) and v != 0)


@pytest.mark.parametrize("model,space", CASES)
def test_successors_and_verdicts_on_mutants(vt, model, space):
    orc, _po = im.MODELS[model]
    R, values, L, _depth = im.SPACES[space]
    fams, _refused = im.families(model, space)
    words = np.concatenate([f.mutant.words for f in fams])
    off = np.cumsum([0] + [len(f.mutant.words) for f in fams]).astype(np.uint64)
    make = vt.Model.second_model if model == 2 else vt.Model.third_model
    P0 = im.oracle_params(model, space, 0)
    want = []                                                           # per parent: {(action, fp, auxkey): (count, verdicts, record)}
    for f in fams:
        d = {}
        for s in f.children:
            key = (s["action"], s["fp"], s["auxkey"])
            n, v, rec = d.get(key, (0, s["verdicts"], None))
            assert v == s["verdicts"]
            d[key] = (n + 1, v, tuple(int(x) for x in orc.normalise(P0, s["words"])))
        want.append(d)
    seen = collections.Counter()
    raising = collections.Counter()
    masks = [im.CFG_MASK[model], im.ALL_MASK[model]] + list(im.BITS[model])
    for mask in masks:
        m = make(R=R, n=len(values), L=L, invariant_mask=mask)
        got = [collections.defaultdict(list) for _ in fams]
        for s in m.get_next_states(words, off):
            assert s["err"] == 0, (fams[s["parent"]].mutant.tag, s["err"])
            got[s["parent"]][(s["action"], s["fp"], s["auxkey"])].append(s)
        for f, g, w in zip(fams, got, want):
            where = (model, space, mask, f.mutant.cls, f.mutant.tag)
            assert {k: len(v) for k, v in g.items()} == {k: v[0] for k, v in w.items()}, where
            for key, ss in g.items():
                _n, verdicts, rec = w[key]
                for s in ss:
                    assert s["inv"] == _expected(verdicts, mask), where + (orc.ACTIONS[key[0]], s["inv"], verdicts)
                    if mask == masks[0]:
                        assert tuple(int(x) for x in orc.normalise(P0, s["words"])) == rec, where
                    if mask in im.BITS[model]:
                        seen[(mask, "set" if s["inv"] else "clear")] += 1
                        if verdicts[mask] == im.RAISES:                 # the documented rule: reported as a violation of the bit
                            assert s["inv"] == mask, where
                            raising[mask] += 1
                    elif mask == masks[0] and any(verdicts[b] == im.RAISES for b in verdicts if b & mask):
                        assert s["inv"] != 0, where
        m.close()
    print("model %d %s: %d parents, kernel verdicts under the single-bit masks %s, of them on an evaluation error %s"
          % (model, space, len(fams), sorted(seen.items()), sorted(raising.items())))
    for b in im.BITS[model]:
        assert seen[(b, "set")] > 0 and seen[(b, "clear")] > 0
    assert raising[4] > 0 and (model == 2 or raising[16] > 0)


@pytest.mark.parametrize("model", [2, 3])
def test_floors(model):
    im.check_floors(model)


@pytest.mark.parametrize("model", [2, 3])
def test_reporting_path_on_a_seeded_level(vt, model, tmp_path):
    """k_expand, the probe and the trace on the clean parents of class E, seeded as level 1 (child process with the hooks library)"""
    out = tmp_path / "out.json"
    env = dict(os.environ, VSRMC_LIB=os.path.join(ROOT, "vsr_tlaplus_amd", "libvsrmc_hooks.so"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "model_seeded_worker.py"), str(model), str(out)],
                       capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(out) as f:
        res = json.load(f)
    assert res["seeds"] >= 100 and res["runs"]
    for b in res["bits_that_occur"] + [im.CFG_MASK[model]]:
        assert sum(run["violators"] for run in res["runs"] if run["mask"] == b) > 0, b
    assert set(res["bits_that_occur"]) >= {2, 4} | ({16} if model == 3 else set())
