"""The regenerating pass over the claim bitmap as a kernel of its own (csrc/vsr_regen_bits.hpp: k_regen_bits) against the CPU oracle.

Every space is searched beyond its record buffers from a low stored base, so that every deepen() after the first regenerates the level above the base
from the claim bitmap, in several slices, three ways: by default (k_regen_bits where the configuration has it), with VSRMC_NO_REGEN_KERNEL=1 (k_expand's
regenerating instantiation) and with VSRMC_REGEN_TRIP=8 (so few instances per trip that nearly every mini-tile takes several and the waves' chunks of the
destination roll over often).  A regenerated state that is lost, doubled or mis-built changes the successors or a checksum of the level above it: every
inserted and every probed level's figures are the same the three ways, and they are the oracle's.

The base levels are chosen so that each place where the kernel can go wrong occurs in at least one space; test_the_chosen_bases_cover_the_edge_cases
derives that from the oracle's levels (and, for what is a matter of ordinals, from the enumeration of the oracle's records in gen<>'s numbering)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
A_SEND_GET_STATE = 13

SMALL = dict(table_log2=20, frontier_words=1 << 21, frontier_states=1 << 15, pending_entries=1 << 16)
# constants (R, C, |Values|, L), invariant mask (None: the default), the stored base level, descents after the first deepen(), checker sizes
SPACES = {
    "3-1-2-1-mask2": dict(c=(3, 1, 2, 1), mask=2, base=13, descents=4, sizes=SMALL),
    "3-1-2-2": dict(c=(3, 1, 2, 2), mask=None, base=7, descents=3, sizes=SMALL),
    "3-1-3-3": dict(c=(3, 1, 3, 3), mask=None, base=6, descents=3, sizes=SMALL),                          # spec 313, the bench's
    "5-1-2-2": dict(c=(5, 1, 2, 2), mask=None, base=4, descents=3, sizes=dict(SMALL, frontier_words=1 << 22), fixture="oracle_levels_config5.json"),   # no k_regen_bits at R = 5: the fallback
}
WAYS = {"default": None, "no-regen-kernel": ("VSRMC_NO_REGEN_KERNEL", "1"), "short-trip": ("VSRMC_REGEN_TRIP", "8")}
KNOBS = ("VSRMC_NO_REGEN_KERNEL", "VSRMC_REGEN_TRIP", "VSRMC_REGEN_DST_STATES", "VSRMC_REGEN_DST_WORDS", "VSRMC_NO_PROBE_KERNEL", "VSRMC_PROBE_LIST", "VSRMC_PROBE_CCAP", "VSRMC_CCAP")
_oracle = {}


def _params(orc, sp):
    R, C_, n, L = sp["c"]
    return orc.Params(R, C_, n, L, invariant_mask=sp["mask"]) if sp["mask"] is not None else orc.Params(R, C_, n, L)


def _last(sp):
    return sp["base"] + 2 + sp["descents"]                        # the deepest probed level: deepen() 1 inserts base + 1; descent k inserts base + 1 + k, probes base + 2 + k


_succ_buf = []
BIG_LEVEL = 20000


def _succ_meta(orc, P, rec):
    """(action, fingerprint, invariant bits) of every successor of `rec`, as three arrays: orc.successors without the copy of every successor's words (the
    R = 5 space has 3.9 M successors at its deepest probed level; only these three figures of each are needed here)"""
    if not _succ_buf:
        _succ_buf.extend((np.zeros(1 << 16, dtype=np.uint64), np.zeros(5 * 512, dtype=np.uint64)))
    words, meta = _succ_buf
    used = C.c_int()
    n = orc.lib().orc_successors(C.c_void_p(P.ptr), C.c_void_p(rec.ctypes.data), C.c_void_p(words.ctypes.data), len(words), C.c_void_p(meta.ctypes.data), 512, C.byref(used))
    assert n >= 0, n
    m = meta[: 5 * n].reshape(n, 5)
    return m[:, 0].astype(np.int64), m[:, 1], m[:, 4]


def _oracle_levels(name):
    """level K -> the oracle's figures of level K as an inserted level and as a probed one (computed once per space, shared, never changed);
    also: the base level's records and the set of fingerprints of the levels up to it"""
    if name in _oracle:
        return _oracle[name]
    from oracle import orc
    sp = SPACES[name]
    P = _params(orc, sp)
    ob = orc.Bfs(P)
    seen = set(int(x) for x in ob.level_fps(1))
    out = dict(levels={}, base=None)
    while ob.info["depth"] < _last(sp):
        lvl = ob.info["depth"]
        words, off = ob.frontier()                                # the states of level `lvl`: the parents of level lvl + 1
        if lvl == sp["base"]:
            out["base"] = (words, off, set(seen))
        act, dead, bad = [0] * 16, 0, {}
        # A level of more than BIG_LEVEL parents costs the oracle too long for a test (the R = 5 space: 4.7 s for level 8, 27 s for level 9): from there on
        # the figures are the ones the same oracle recorded in its committed fixture — which the levels computed here must equal too
        if "fixture" in sp and len(off) - 1 > BIG_LEVEL:
            break
        if lvl + 1 > sp["base"]:
            words = np.ascontiguousarray(words, dtype=np.uint64)
            acc = np.zeros(16, dtype=np.int64)
            for i in range(len(off) - 1):
                a_, fp_, inv_ = _succ_meta(orc, P, words[int(off[i]): int(off[i + 1])])
                dead += 0 if len(a_) else 1
                acc += np.bincount(a_, minlength=16)[:16]
                for k in np.nonzero(inv_)[0]:
                    if int(fp_[k]) not in seen:
                        bad[int(fp_[k])] = bad.get(int(fp_[k]), 0) | int(inv_[k])
            act = [int(x) for x in acc]
        nn = ob.step()
        assert nn > 0, (name, lvl)
        fps = ob.level_fps(lvl + 1)
        seen.update(int(x) for x in fps)
        mask = 0
        for v in bad.values():
            mask |= v
        if lvl + 1 > sp["base"]:
            assert mask == ob.info["viol_mask"], (name, lvl + 1)
            assert (sum(act), dead) == (ob.info["generated"], ob.info["deadlocks"]), (name, lvl + 1)
            out["levels"][lvl + 1] = dict(n_new=nn, generated=sum(act), act_generated=act[1:16], deadlocks=dead, max_bag=ob.info["max_bag"],
                                          fp_xor=int(np.bitwise_xor.reduce(fps)), fp_sum=int(fps.astype(object).sum()) & M64,
                                          viol_mask=mask, viol_fp=min(bad) if bad else None)
    ob.close()
    if "fixture" in sp:
        with open(os.path.join(os.path.dirname(__file__), "golden", sp["fixture"])) as f:
            g = json.load(f)
        assert g["viol_mask"] == 0 and [g["params"][k] for k in ("R", "C", "n", "L")] == list(sp["c"])
        for lv in g["levels"]:
            if sp["base"] < lv["level"] <= _last(sp):
                w = dict(n_new=lv["new"], generated=lv["generated"], act_generated=lv["act_generated"][1:16], deadlocks=lv["deadlocks"], max_bag=lv["max_bag"],
                         fp_xor=int(lv["fp_xor"], 16), fp_sum=int(lv["fp_sum"], 16), viol_mask=0, viol_fp=None)
                assert out["levels"].setdefault(lv["level"], w) == w, (name, lv["level"])
    assert sorted(out["levels"]) == list(range(sp["base"] + 1, _last(sp) + 1)), (name, sorted(out["levels"]))
    _oracle[name] = out
    return out


def _run(name, way, monkeypatch, sizes=None):
    import vsr_tlaplus_amd as vt
    sp = SPACES[name]
    for var in KNOBS:
        monkeypatch.delenv(var, raising=False)
    if WAYS[way]:
        monkeypatch.setenv(*WAYS[way])
    R, C_, n, L = sp["c"]
    kw = dict(invariant_mask=sp["mask"]) if sp["mask"] is not None else {}
    m = vt.Model.from_constants(R=R, C_=C_, n=n, L=L, **kw)
    mc = vt.ModelChecker(m, **(sizes or sp["sizes"]))             # (the environment is read when the checker is created)
    for _ in range(sp["base"] - 1):
        mc.step()
    assert mc.level == sp["base"]
    inserted, probed, slices = {}, {}, []
    for k in range(sp["descents"] + 1):
        a, b = mc.deepen()
        inserted[a["level"]] = dict(n_new=a["n_new"], generated=a["generated"], act_generated=[int(x) for x in a["act_generated"][1:16]], deadlocks=a["deadlocks"],
                                    max_bag=a["max_bag"], fp_xor=a["fp_xor"], fp_sum=a["fp_sum"], viol_mask=a["viol_mask"],
                                    viol_fp=a["viol_fp"] if a["viol_mask"] else None)
        if k == 0:                                                # the first pass inserts the level above the base as a virtual level: nothing regenerated, nothing probed
            assert b is None and a["materialize_ms"] == 0.0
            continue
        assert a["materialize_ms"] > 0.0                          # a descent: the bitmap level was regenerated
        slices.append(a["words_new"] >> 32)
        if a["viol_mask"]:
            break
        assert b is not None and b["level"] == a["level"] + 1
        probed[b["level"]] = dict(generated=b["generated"], act_generated=[int(x) for x in b["act_generated"][1:16]], deadlocks=b["deadlocks"], viol_mask=b["viol_mask"],
                                  viol_fp=b["viol_fp"] if b["viol_mask"] else None)
        if b["viol_mask"]:
            break
    launches = mc.regen_launches()
    mc.close()
    return dict(inserted=inserted, probed=probed, slices=slices, launches=launches)


def _held_against_the_oracle(name, way, got, want):
    for lvl, d in got["inserted"].items():
        print(name, way, "inserted", lvl, d["n_new"], d["generated"], d["deadlocks"], d["max_bag"], "%016x" % d["fp_xor"], d["viol_mask"])
        assert d == want[lvl], (name, way, lvl, d, want[lvl])
    for lvl, d in got["probed"].items():
        w = {k: want[lvl][k] for k in d}
        print(name, way, "probed", lvl, d["generated"], d["deadlocks"], d["viol_mask"])
        assert d == w, (name, way, lvl, d, w)


@pytest.mark.parametrize("name", list(SPACES))
def test_regenerated_levels_equal_three_ways_and_the_oracle(name, monkeypatch):
    want = _oracle_levels(name)["levels"]
    sp = SPACES[name]
    runs = {way: _run(name, way, monkeypatch) for way in WAYS}
    for way, got in runs.items():
        assert len(got["slices"]) >= 3 or any(d["viol_mask"] for d in list(got["inserted"].values()) + list(got["probed"].values())), (way, got["slices"])
        assert all(s >= 2 for s in got["slices"]), (way, got["slices"])          # several slices per descent: all but the first start at p_offset != 0
        _held_against_the_oracle(name, way, got, want)
        assert got["inserted"] == runs["default"]["inserted"] and got["probed"] == runs["default"]["probed"], way
    print(name, "k_regen_bits launches", {way: got["launches"] for way, got in runs.items()})
    assert runs["no-regen-kernel"]["launches"] == 0
    if sp["c"][0] <= 3:                                           # did the new kernel run?
        assert runs["default"]["launches"] >= sum(runs["default"]["slices"]) > 0 and runs["short-trip"]["launches"] > 0
    else:
        assert runs["default"]["launches"] == 0 and runs["short-trip"]["launches"] == 0


def test_a_small_destination_completes(monkeypatch):
    """Record buffers of 2^17 words and 2^12 states: the descents' scratch slices are a few hundred parents, the waves' chunks shrink to their smallest sizes
    and the destination has room for little more than four chunks per wave.  The slices are sized to fit, so no pass runs full: the search completes with the
    oracle's figures, by the kernel of its own as by k_expand's instantiation."""
    name = "3-1-2-2"
    want = _oracle_levels(name)["levels"]
    sizes = dict(SMALL, frontier_words=1 << 17, frontier_states=1 << 12)
    res = {way: _run(name, way, monkeypatch, sizes=sizes) for way in ("default", "no-regen-kernel")}
    for way, got in res.items():
        print(way, got["slices"], got["launches"])
        _held_against_the_oracle(name, way, got, want)
    assert res["default"]["launches"] > 0 and res["no-regen-kernel"]["launches"] == 0


@pytest.mark.parametrize("knob", [("VSRMC_REGEN_DST_STATES", "4096"), ("VSRMC_REGEN_DST_WORDS", "131072")])
def test_a_slice_that_runs_full_is_refused_the_same_way(knob, monkeypatch):
    """A regenerating slice that really runs into the end of its destination (LevelCtl::full: the index chunks, then the word chunks).  The slices of a descent
    are sized to fit their buffer, so the knob hands the regenerating pass less of it than the slice was sized for: (3,1,{v1,v2},2) from base 10 regenerates
    the 43 306 states of level 11 in slices of several thousand children, 4 096 indices / 131 072 words hold none of them.  A full slice loses records, so it
    is an error of the pass on either path (pass_verdict: ERR_FRONTIER_FULL) — the search does NOT complete; what is asserted is that the kernel of its own
    keeps writing inside the buffer, ends, and is refused exactly as k_expand's instantiation is: the same code, device error and level, in the same descent."""
    import vsr_tlaplus_amd as vt
    got = {}
    for way in ("default", "no-regen-kernel"):
        for var in KNOBS:
            monkeypatch.delenv(var, raising=False)
        if WAYS[way]:
            monkeypatch.setenv(*WAYS[way])
        monkeypatch.setenv(*knob)
        m = vt.Model.from_constants(R=3, C_=1, n=2, L=2)
        mc = vt.ModelChecker(m, **SMALL)
        for _ in range(9):
            mc.step()
        assert mc.level == 10
        a, b = mc.deepen()                                        # level 11 as a virtual level: nothing is regenerated yet
        assert (a["level"], a["n_new"], b) == (11, 43306, None)
        with pytest.raises(vt.VsrmcError) as e:
            mc.deepen()                                           # the first descent: its first regenerating slices run full
        err = re.search(r"device error (\d+) at .* \(level (\d+)\)", e.value.message)
        assert err, e.value.message
        got[way] = (e.value.code, int(err.group(1)), int(err.group(2)), mc.regen_launches())
        print(knob, way, got[way], e.value.message)
        mc.close()
    assert got["default"][:3] == got["no-regen-kernel"][:3] and got["default"][2] == 11
    assert got["default"][3] > 0 and got["no-regen-kernel"][3] == 0   # the default path got there through k_regen_bits


def test_the_chosen_bases_cover_the_edge_cases():
    """Parent counts that are no multiple of 16; a stored level whose index range ends in holes; parents without a set bit; set bits beyond the first bitmap
    word; message-bound ordinals with k2 = 0 and with k2 != 0; children longer than their parent.  The states and which successors are new come from the
    oracle; an instance's ordinal is the position gen<> gives it (Model.get_next_states on the oracle's records: the numbering is the library's own)."""
    import vsr_tlaplus_amd as vt
    from oracle import orc
    seen_cases = dict(not_mult_16=False, holes=False, no_bit=False, beyond_word_0=False, k2_zero=False, k2_nonzero=False, longer_child=False)
    for name, sp in SPACES.items():
        if sp["c"][0] > 3:
            continue
        R, C_, n, L = sp["c"]
        words, off, seen = _oracle_levels(name)["base"]
        n_par = len(off) - 1
        seen_cases["not_mult_16"] |= n_par % 16 != 0
        seen_cases["holes"] |= n_par % 2048 != 0                  # k_expand hands indices out in chunks of at least 2048 (VSR_CAND_CAP) and leaves a chunk's tail as invalid refs
        kw = dict(invariant_mask=sp["mask"]) if sp["mask"] is not None else {}
        m = vt.Model.from_constants(R=R, C_=C_, n=n, L=L, **kw)
        m0 = 4 * R + R * C_ * n
        first = {}                                                # new state -> does any parent reach it (a bit is set for exactly one of its instances)
        per_parent = [0] * n_par
        for s in m.get_next_states(words, off):
            if s["fp"] in seen:
                continue
            per_parent[s["parent"]] += 1
            plen = int(off[s["parent"] + 1] - off[s["parent"]])
            # a state every one of whose instances has the property has its one set bit at such an instance
            p = first.setdefault(s["fp"], dict(beyond=True, k2z=True, k2n=True, longer=True))
            p["beyond"] &= s["ordinal"] >= 32
            p["k2z"] &= s["ordinal"] >= m0 and (s["ordinal"] - m0) % (R + 1) == 0
            p["k2n"] &= s["ordinal"] >= m0 and (s["ordinal"] - m0) % (R + 1) != 0 and s["action"] == A_SEND_GET_STATE
            p["longer"] &= len(s["words"]) > plen
        seen_cases["no_bit"] |= any(c == 0 for c in per_parent)
        seen_cases["beyond_word_0"] |= any(p["beyond"] for p in first.values())
        seen_cases["k2_zero"] |= any(p["k2z"] for p in first.values())
        seen_cases["k2_nonzero"] |= any(p["k2n"] for p in first.values())
        seen_cases["longer_child"] |= any(p["longer"] for p in first.values())
        print(name, n_par, {k: v for k, v in seen_cases.items()})
    assert all(seen_cases.values()), seen_cases
