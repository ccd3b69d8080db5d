"""The probe pass as kernels of its own (csrc/vsr_probe_scan.hpp: k_probe_scan + k_probe_apply + k_probe_resolve) against the CPU oracle.

Every space is searched beyond its record buffers from a low base, so that several probe passes happen, three ways: by default (the scan
kernel), with VSRMC_NO_PROBE_KERNEL=1 (the mode-capable k_expand) and with VSRMC_PROBE_LIST=8 (a list of footprint instances so short that
the pass overflows it and is run again by the mode-capable kernel).  Every probed level's figures — successors in total and per action,
deadlocks, the violated invariants, the smallest violating fingerprint, the sorted list of violating states — are the same the three
ways, and they are what the oracle gets by expanding the level's parents one by one."""
import pytest

pytestmark = pytest.mark.gpu

# constants (R, C, |Values|, L), invariant mask (None: the default), the stored base level, the last probed level (the first is base + 3), checker sizes
SPACES = {
    "3-1-2-1-mask2": dict(c=(3, 1, 2, 1), mask=2, base=13, upto=19, sizes=dict(table_log2=20, frontier_words=1 << 21, frontier_states=1 << 15, pending_entries=1 << 16)),
    "3-1-2-2": dict(c=(3, 1, 2, 2), mask=None, base=7, upto=12, sizes=dict(table_log2=20, frontier_words=1 << 21, frontier_states=1 << 15, pending_entries=1 << 16)),
    "3-1-3-3-prefix": dict(c=(3, 1, 3, 3), mask=None, base=6, upto=11, sizes=dict(table_log2=20, frontier_words=1 << 21, frontier_states=1 << 15, pending_entries=1 << 16)),
    "5-1-2-2-prefix": dict(c=(5, 1, 2, 2), mask=None, base=4, upto=9, sizes=dict(table_log2=20, frontier_words=1 << 22, frontier_states=1 << 15, pending_entries=1 << 16)),
}
WAYS = {"default": None, "no-probe-kernel": ("VSRMC_NO_PROBE_KERNEL", "1"), "short-list": ("VSRMC_PROBE_LIST", "8")}
_oracle = {}


def _params(orc, sp):
    R, C_, n, L = sp["c"]
    return orc.Params(R, C_, n, L, invariant_mask=sp["mask"]) if sp["mask"] is not None else orc.Params(R, C_, n, L)


def _oracle_probes(name):
    """probed level K -> what expanding every state of level K - 1 gives (successors already seen at a level < K are dropped, like TLC drops them)"""
    if name in _oracle:
        return _oracle[name]
    from oracle import orc
    sp = SPACES[name]
    P = _params(orc, sp)
    ob = orc.Bfs(P)
    seen = set(int(x) for x in ob.level_fps(1))
    out = {}
    while ob.info["depth"] < sp["upto"] - 1:
        assert ob.step() > 0
        lvl = ob.info["depth"]
        seen.update(int(x) for x in ob.level_fps(lvl))
        if lvl + 1 < sp["base"] + 3:
            continue
        words, off = ob.frontier()
        act = [0] * 16
        dead = 0
        bad = {}
        for i in range(len(off) - 1):
            succ = orc.successors(P, words[int(off[i]): int(off[i + 1])])
            dead += 0 if succ else 1
            for s in succ:
                act[s["action"]] += 1
                if s["inv"] and s["fp"] not in seen:
                    bad[s["fp"]] = bad.get(s["fp"], 0) | s["inv"]
        mask = 0
        for v in bad.values():
            mask |= v
        out[lvl + 1] = dict(generated=sum(act), act_generated=act[1:16], deadlocks=dead, viol_mask=mask, viol_fp=min(bad) if bad else None, violators=sorted(bad))
    ob.close()
    _oracle[name] = out
    return out


def _run(name, way, monkeypatch):
    import vsr_tlaplus_amd as vt
    sp = SPACES[name]
    for var in ("VSRMC_NO_PROBE_KERNEL", "VSRMC_PROBE_LIST", "VSRMC_PROBE_CCAP"):
        monkeypatch.delenv(var, raising=False)
    if WAYS[way]:
        monkeypatch.setenv(*WAYS[way])
    R, C_, n, L = sp["c"]
    kw = dict(invariant_mask=sp["mask"]) if sp["mask"] is not None else {}
    m = vt.Model.from_constants(R=R, C_=C_, n=n, L=L, **kw)
    mc = vt.ModelChecker(m, **sp["sizes"])                      # (the environment is read when the checker is created)
    for _ in range(sp["base"] - 1):
        mc.step()
    assert mc.level == sp["base"]
    got = {}
    launches = 0
    while True:
        a, b = mc.deepen()
        launches += a["pending"]
        assert a["viol_mask"] == 0, a["level"]
        if a["level"] == sp["base"] + 1:                         # the first pass inserts the level above the base as a virtual level and probes nothing
            assert b is None
            continue
        assert b is not None and b["level"] == a["level"] + 1
        got[b["level"]] = dict(generated=b["generated"], act_generated=[int(x) for x in b["act_generated"][1:16]], deadlocks=b["deadlocks"], viol_mask=b["viol_mask"],
                               viol_fp=b["viol_fp"] if b["viol_mask"] else None, violators=mc.probe_violators() if b["viol_mask"] else [])
        if b["level"] >= sp["upto"] or b["viol_mask"]:
            break
    mc.close()
    return got, launches


@pytest.mark.parametrize("name", list(SPACES))
def test_probed_levels_equal_three_ways_and_the_oracle(name, monkeypatch):
    want = _oracle_probes(name)
    sp = SPACES[name]
    runs = {way: _run(name, way, monkeypatch) for way in WAYS}
    levels = list(range(sp["base"] + 3, sp["upto"] + 1))
    assert len(levels) >= 3                                       # several probe passes
    for way, (got, _launches) in runs.items():
        assert sorted(got) == levels, (way, sorted(got))
        for lvl in levels:
            print(name, way, lvl, got[lvl]["generated"], got[lvl]["deadlocks"], got[lvl]["viol_mask"], len(got[lvl]["violators"]))
            assert got[lvl] == want[lvl], (name, way, lvl, got[lvl], want[lvl])
    if sp["mask"] is not None:                                    # (3,1,{v1,v2},1), AcknowledgedWritesExistOnMajority: the violation at depth 19 is inside the probed range
        assert want[19]["viol_mask"] == 2 and want[19]["violators"]
    if sp["c"][0] <= 3:                                           # the short list made passes overflow: each of them ran a third kernel launch and more
        assert runs["short-list"][1] > runs["default"][1], (runs["short-list"][1], runs["default"][1])
