"""The host model of the seen-set (tests/seen_set_model.py) against itself: its key generators deliver what they promise, its claims do not depend on
order or batching, its invariant checker rejects bad tables, its meta helpers agree with the layout of csrc/vsr_model.hpp.  No GPU."""
import numpy as np

import seen_set_model as sm


def test_meta_word_layout_and_round_trip():
    # csrc/vsr_model.hpp: level(9) << 55 | canonical auxkey(9) << 46 | low 45 bits of the PARENT's fingerprint << 1 | taken(1)
    assert sm.meta_make(23, 0x155, 0xFEDCBA9876543210) == 0x0BD57530ECA86420
    assert sm.meta_make(23, 0x155, 0xFEDCBA9876543210) == (23 << 55) | (0x155 << 46) | ((0xFEDCBA9876543210 & ((1 << 45) - 1)) << 1)
    assert sm.META_EMPTY == 0xFFFFFFFFFFFFFFFF and sm.META_TAKEN == 1 and sm.meta_level(sm.META_EMPTY) == 511
    rng = np.random.default_rng(1)
    for _ in range(200):
        lv, ak, pf = int(rng.integers(0, 512)), int(rng.integers(0, 512)), int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        m = sm.meta_make(lv, ak, pf)
        assert m & 1 == 0 and m < 1 << 64
        for t in (m, m | sm.META_TAKEN):
            assert (sm.meta_level(t), sm.meta_auxkey(t), sm.meta_pfp(t)) == (lv, ak, pf & sm.PFP_MASK)
    # smaller = wins: level first, then auxkey, then parent bits
    assert sm.meta_make(3, 511, sm.PFP_MASK) < sm.meta_make(4, 0, 0) and sm.meta_make(4, 1, sm.PFP_MASK) < sm.meta_make(4, 2, 0)
    assert sm.owner_of(0x0000_0300_0000_0000, 8) == 3 and sm.owner_of(0xFFFF_FF00_0000_0000 | 12345, 3) == 0xFFFFFF % 3


def test_probe_reach_of_every_start_inside_a_line():
    assert [sm.probe_reach(h) for h in range(4)] == [8192, 8191, 8190, 8193]
    assert min(sm.probe_reach(h) for h in range(64)) == 1 + 2048 * 4 - 3


def test_cluster_generators():
    for log2, home, n, extra in ((8, 0, 192, 0), (8, 255, 192, 2), (10, 1019, 768, 1), (15, 32762, 8256, 0), (4, 0, 25, 0)):
        fps = sm.cluster(log2, home, n, extra_equal_bits=extra, seed=5)
        assert fps.dtype == np.uint64 and len(fps) == n and len(set(int(f) for f in fps)) == n and (fps != 0).all()
        mask = (1 << log2) - 1
        assert all(int(f) & mask == home for f in fps)
        assert len({(int(f) >> log2) & ((1 << extra) - 1) for f in fps}) == 1          # the extra bits agree ...
        assert len({int(f) & ((1 << (log2 + extra)) - 1) for f in fps}) == 1           # ... so `extra` doublings leave one home
        if n >= 60:
            assert len({int(f) & ((1 << (log2 + extra + 1)) - 1) for f in fps}) == 2   # ... and one more splits the cluster
        assert np.array_equal(fps, sm.cluster(log2, home, n, extra_equal_bits=extra, seed=5))       # deterministic
        assert not np.array_equal(fps, sm.cluster(log2, home, n, extra_equal_bits=extra, seed=6))
    for log2, home, n, extra in ((8, 254, 80, 0), (8, 3, 25, 1), (10, 0, 300, 2)):
        fps = sm.wset_cluster(log2, home, n, extra_equal_bits=extra, seed=5)
        assert len(set(int(f) for f in fps)) == n and (fps != 0).all()
        assert all(sm.wset_home(int(f), (1 << log2) - 1) == home for f in fps)
        assert len({sm.wset_home(int(f), (1 << (log2 + extra)) - 1) for f in fps}) == 1
        assert len({int(f) & 0x1FFF for f in fps}) > 1                                # the bits below the home bits vary
        assert len({int(f) & ((1 << log2) - 1) for f in fps}) > 1                     # (so the seen-set's own home differs)


def test_same_low45():
    fp = 0x123456789ABCDEF1
    out = sm.same_low45(fp, 5)
    assert len(set(int(f) for f in out)) == 5 and fp not in {int(f) for f in out}
    assert all(int(f) & sm.PFP_MASK == fp & sm.PFP_MASK for f in out)


def test_dup_batch_multiplicities_and_kinds():
    fps = sm.cluster(10, 1021, 200, seed=2)
    b = sm.dup_batch(fps, 6, seed=3, pad=37)
    assert b.shape[1] == 2 and b.dtype == np.uint64
    rows = sm.batch_list(b)
    assert sum(1 for f, k in rows if f == 0) == 37 and all(k == 0 for f, k in rows if f == 0)
    groups = {}
    for f, k in rows:
        if f:
            groups.setdefault(f, []).append(k)
    assert set(groups) == {int(f) for f in fps}
    mult = {len(v) for v in groups.values()}
    assert min(mult) >= 1 and max(mult) <= 7 and len(mult) == 7
    kinds = {"aux": 0, "pfp": 0, "same": 0}
    for i, f in enumerate(fps):
        keys = groups[int(f)]
        assert all(sm.meta_level(k) == 6 and k & 1 == 0 for k in keys)
        if len(keys) > 1:
            if len({sm.meta_auxkey(k) for k in keys}) == len(keys):
                kinds["aux"] += 1
                assert len({sm.meta_pfp(k) for k in keys}) == 1
            elif len({sm.meta_pfp(k) for k in keys}) == len(keys):
                kinds["pfp"] += 1
                assert len({sm.meta_auxkey(k) for k in keys}) == 1
            else:
                kinds["same"] += 1
                assert len(set(keys)) == 1
    assert min(kinds.values()) > 20
    # shuffled: the candidates of one fingerprint are not all adjacent
    pos = {}
    for i, (f, _k) in enumerate(rows):
        pos.setdefault(f, []).append(i)
    assert any(max(p) - min(p) >= len(p) for f, p in pos.items() if f and len(p) > 1)
    assert np.array_equal(b, sm.dup_batch(fps, 6, seed=3, pad=37))


def _state():
    old = sm.cluster(10, 1021, 100, seed=1)
    new = sm.cluster(10, 1021, 150, seed=2)
    t5 = sm.claim_fused({}, [(int(f), sm.meta_make(5, i % 512, i)) for i, f in enumerate(old)], 5)
    batch = sm.batch_list(sm.dup_batch(np.concatenate([new, old[::2]]), 6, seed=4, parents=old, pad=11))
    return t5, batch


def test_the_claim_model_does_not_depend_on_order_or_batching():
    t5, batch = _state()
    rng = np.random.default_rng(8)
    for claim in (sm.claim_exact, sm.claim_fused):
        ref = claim(t5, batch, 6)
        for f, m in t5.items():
            assert ref[f] == m                                      # the states of level 5 keep their meta words
        for _ in range(5):
            perm = [batch[i] for i in rng.permutation(len(batch))]
            assert claim(t5, perm, 6) == ref
            cut = int(rng.integers(1, len(batch) - 1))
            assert claim(claim(t5, perm[:cut], 6), perm[cut:], 6) == ref
    exact, fused = sm.claim_exact(t5, batch, 6), sm.claim_fused(t5, batch, 6)
    for f in exact:
        if f in t5:
            assert exact[f] == fused[f] == t5[f]
        else:
            keys = [k for g, k in batch if g == f]
            assert fused[f] == min(keys) and exact[f] == min(keys) | sm.META_TAKEN
    assert 0 not in exact and 0 not in fused


def test_the_verdict_checkers_accept_the_rule_and_reject_its_violations():
    t5, batch = _state()
    best, ver = {}, [0] * len(batch)
    for i, (f, k) in enumerate(batch):
        if f and f not in t5 and (f not in best or k < batch[best[f]][1]):
            best[f] = i
    for i in best.values():
        ver[i] = 1
    assert sm.check_exact_verdicts(t5, batch, 6, ver) is None
    assert sm.fused_ties_expected(t5, batch)
    assert sm.check_fused_verdicts(t5, batch, 6, ver, 3) is None
    assert "ties" in sm.check_fused_verdicts(t5, batch, 6, ver, 0)
    i_win = next(iter(best.values()))
    v = list(ver); v[i_win] = 0
    assert "0 winners" in sm.check_exact_verdicts(t5, batch, 6, v) and "0 winners" in sm.check_fused_verdicts(t5, batch, 6, v, 1)
    f_multi = next(f for f, k in batch if f and f not in t5 and sum(1 for g, _ in batch if g == f) > 1 and len({kk for g, kk in batch if g == f}) > 1)
    others = [i for i, (g, k) in enumerate(batch) if g == f_multi and i != best[f_multi]]
    v = list(ver); v[others[0]] = 1
    assert "2 winners" in sm.check_exact_verdicts(t5, batch, 6, v)
    v = list(ver); v[best[f_multi]] = 0; v[[i for i in others if batch[i][1] != batch[best[f_multi]][1]][0]] = 1
    assert "smallest key" in sm.check_exact_verdicts(t5, batch, 6, v)
    assert sm.check_fused_verdicts(t5, batch, 6, v, 1) is None      # the single-pass scheme does not say which candidate wins
    i_old = next(i for i, (f, k) in enumerate(batch) if f in t5)
    v = list(ver); v[i_old] = 1
    assert "won again" in sm.check_exact_verdicts(t5, batch, 6, v) and "won again" in sm.check_fused_verdicts(t5, batch, 6, v, 1)
    i_pad = next(i for i, (f, k) in enumerate(batch) if f == 0)
    v = list(ver); v[i_pad] = 1
    assert "padding" in sm.check_fused_verdicts(t5, batch, 6, v, 1)
    # the level claimed again after untake: every state is granted once more, by the same rule
    after = sm.untake(sm.claim_exact(t5, batch, 6), 6)
    assert sm.check_exact_verdicts(after, batch, 6, ver) is None and sm.claim_exact(after, batch, 6) == sm.claim_exact(t5, batch, 6)
    assert "0 winners" in sm.check_exact_verdicts(after, batch, 6, [0] * len(batch))
    assert "taken already" in sm.check_exact_verdicts(sm.claim_exact(t5, batch, 6), batch, 6, ver)
    # no ties expected when every fingerprint's candidates share the auxkey
    same_aux = [(f, sm.meta_make(6, 9, k)) for f, k in batch if f and f not in t5]
    assert not sm.fused_ties_expected(t5, same_aux)


def _place(S, fps):
    """linear probing by the book, for the invariant checker's positive case"""
    tab = np.zeros(S, dtype=np.uint64)
    for f in fps:
        i = int(f) & (S - 1)
        while tab[i] != 0:
            i = (i + 1) & (S - 1)
        tab[i] = f
    return tab


def test_the_probing_invariant_checker():
    S = 256
    fps = np.concatenate([sm.cluster(8, 253, 40, seed=1), sm.cluster(8, 3, 30, seed=2), sm.cluster(8, 100, 5, seed=3)])
    tab = _place(S, fps)
    metas = np.where(tab != 0, np.uint64(sm.meta_make(2, 1, 7)), np.uint64(sm.META_EMPTY))
    assert sm.check_probing(tab, metas) is None
    assert tab[255] != 0 and tab[0] != 0 and tab[20] != 0                           # the run of home 253 wraps
    model = {int(f): sm.meta_make(2, 1, 7) for f in fps}
    assert sm.compare_dump(tab, metas, model) is None
    # a hole before an entry
    bad = tab.copy(); bad[1] = 0
    msg = sm.check_probing(bad, metas)
    assert msg and "cut off" in msg
    # an entry before its home slot
    bad = tab.copy(); f = bad[102]; bad[102] = 0; bad[99] = f
    assert "cut off" in sm.check_probing(bad, metas)
    # a doubled fingerprint
    bad = tab.copy(); bad[110] = bad[101]
    assert "occurs 2 times" in sm.check_probing(bad, metas)
    # content differences: a meta word, a missing and an extra fingerprint
    m2 = metas.copy(); m2[101] |= np.uint64(1)
    assert "model" in sm.compare_dump(tab, m2, model)
    less = dict(model); gone = less.popitem()
    assert "%016x" % gone[0] in sm.compare_dump(tab, metas, less)
    more = dict(model); more[0xABCDEF] = 5
    assert "nothing" in sm.compare_dump(tab, metas, more)
    # the winner set's home function
    wf = sm.wset_cluster(8, 254, 20, seed=4)
    wt = np.zeros(S, dtype=np.uint64)
    for k, f in enumerate(wf):
        wt[(254 + k) & 255] = f
    assert sm.check_probing(wt, None, home_of=sm.wset_home) is None and sm.check_probing(wt) is not None


def test_level_checksum_untake_seen_walk_and_winner_set():
    t = {5: sm.meta_make(1, 0, 0), 9: sm.meta_make(2, 3, 5) | 1, 12: sm.meta_make(2, 1, 5), (1 << 45) | 9: sm.meta_make(3, 0, 9) | 1}
    assert sm.level_checksum(t, 2) == (9 ^ 12, 21, 2) and sm.level_checksum(t, 7) == (0, 0, 0)
    u = sm.untake(t, 3)
    assert u[9] == t[9] and u[(1 << 45) | 9] == t[(1 << 45) | 9] & ~1 and sm.untake(t, 1)[9] == t[9] & ~1
    assert sm.seen_below(t, [5, 9, 77], 2) == [1, 0, 0]
    assert sm.walk(t, (1 << 45) | 9, 3) == (0, [5, 9, (1 << 45) | 9])
    assert sm.walk(t, 12, 2) == (0, [5, 12]) and sm.walk(t, 12, 3)[0] == 1 and sm.walk(t, 4711, 2)[0] == 1
    t2 = dict(t); t2[(7 << 45) | 9] = sm.meta_make(2, 0, 5)                          # a second level-2 state with the 45 bits of state 9
    assert sm.walk(t2, (1 << 45) | 9, 3)[0] == 2 | (2 << 8) | (2 << 16)
    t3 = dict(t); t3[(7 << 45) | 9] = sm.meta_make(4, 0, 5)                          # ... of another level: ignored
    assert sm.walk(t3, (1 << 45) | 9, 3)[0] == 0
    t4 = dict(t); del t4[5]
    assert sm.walk(t4, 12, 2)[0] == 1
    w = sm.WinnerSet()
    w.insert(100, 6); w.insert(200, 7); w.insert(100, 9)                             # (a state is inserted once: the first level stays)
    assert w.take(100, 6, 1) and not w.take(100, 6, 1) and not w.take(100, 7, 2) and not w.take(300, 6, 2)
    assert w.take(100, 6, 2) and w.take(200, 7, 2) and not w.take(200, 7, 2) and w.take(200, 7, 3)
    assert w.take_batch_counts([100, 100, 300, 200], 6, 5) == {100: 1, 300: 0, 200: 0}
    assert w.words() == {100: (6 << 23) | 5, 200: (7 << 23) | 3}
    w.export_import()
    assert w.words() == {100: 6 << 23, 200: 7 << 23} and w.take(100, 6, 1)
