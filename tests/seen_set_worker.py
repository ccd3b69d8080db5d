"""Child process of tests/test_seen_set_directed.py: drives the seen-set kernels, the winner set and k_partition through the test hooks of
libvsrmc_hooks.so (csrc/host_test_table.hpp; VSRMC_LIB points here) with the adversarial keys of tests/seen_set_model.py, and compares raw dumps,
verdict bytes and side outputs with that model.  One sub-command per test:  python seen_set_worker.py <name>  prints OK, or the first mismatch
(fingerprint, slot, both meta words) and exits 1."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seen_set_model as sm                      # noqa: E402
import vsr_tlaplus_amd as vt                     # noqa: E402
from vsr_tlaplus_amd import capi                 # noqa: E402


class Mismatch(Exception):
    pass


def need(cond, msg):
    if not cond:
        raise Mismatch(msg)


def none(bad):
    if bad:
        raise Mismatch(bad)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


class Table:
    """the seen-set of an ordinary checker, emptied; every method is one hook call"""

    def __init__(self, log2):
        self.lib = capi.load()
        need(hasattr(self.lib, "vsrmc_test_table_claim"), "the loaded library has no test hooks (VSRMC_LIB)")
        self.model = vt.Model.from_constants(R=2, C_=1, n=1, L=1)
        self.mc = vt.ModelChecker(self.model, device=0, table_log2=log2, frontier_words=1 << 16, frontier_states=1 << 12, pending_entries=1 << 14)
        self.h = self.mc._h
        self.clear()

    def clear(self):
        capi.check(self.lib.vsrmc_test_table_clear(self.h))

    def claim(self, entries, level, scheme):
        e = u64(entries).reshape(-1, 2)
        ver = np.zeros(len(e), dtype=np.uint8)
        ctl = np.zeros(3, dtype=np.uint64)
        capi.check(self.lib.vsrmc_test_table_claim(self.h, _p(e), len(e), level, scheme, _p(ver), _p(ctl)))
        return ver, {"err": int(ctl[0]), "ties": int(ctl[1]), "probes": int(ctl[2])}

    def dump(self):
        n = C.c_uint64()
        capi.check(self.lib.vsrmc_test_table_dump(self.h, None, 0, C.byref(n)))
        raw = np.zeros(2 * n.value, dtype=np.uint64)
        capi.check(self.lib.vsrmc_test_table_dump(self.h, _p(raw), n.value, C.byref(n)))
        raw = raw.reshape(-1, 2)
        return raw[:, 0].copy(), raw[:, 1].copy()

    def slots(self):
        n = C.c_uint64()
        capi.check(self.lib.vsrmc_test_table_dump(self.h, None, 0, C.byref(n)))
        return n.value

    def grow(self):
        capi.check(self.lib.vsrmc_test_table_grow(self.h))

    def untake(self, min_level):
        capi.check(self.lib.vsrmc_test_table_untake(self.h, min_level))

    def level_checksum(self, level):
        out = np.zeros(3, dtype=np.uint64)
        capi.check(self.lib.vsrmc_test_table_level_checksum(self.h, level, _p(out)))
        return tuple(int(v) for v in out)

    def lookup(self, key, level, by_low_bits):
        found, fp, meta = C.c_int32(), C.c_uint64(), C.c_uint64()
        capi.check(self.lib.vsrmc_test_table_lookup(self.h, C.c_uint64(int(key)), level, int(by_low_bits), C.byref(found), C.byref(fp), C.byref(meta)))
        return found.value, fp.value, meta.value

    def walk(self, fp, level):
        raw = np.zeros(level + 1, dtype=np.uint64)
        fps = np.zeros(level, dtype=np.uint64)
        rc = C.c_int32()
        capi.check(self.lib.vsrmc_test_table_walk(self.h, C.c_uint64(int(fp)), level, _p(raw), _p(fps), C.byref(rc)))
        return int(raw[level]), [int(v) for v in raw[:level]], rc.value, [int(v) for v in fps], self.lib.vsrmc_last_error().decode()

    def probe_lookup(self, fps):
        f = u64(fps)
        found = np.zeros(len(f), dtype=np.uint8)
        metas = np.zeros(len(f), dtype=np.uint64)
        capi.check(self.lib.vsrmc_test_table_probe_lookup(self.h, _p(f), len(f), _p(found), _p(metas)))
        return found, metas

    def seen_batch(self, fps, level):
        f = u64(fps)
        out = np.full(len(f), 0xEE, dtype=np.uint8)
        capi.check(self.lib.vsrmc_checker_seen_batch(self.h, _p(f), len(f), level, _p(out)))
        return out

    def export_import(self, window, new_log2):
        n = C.c_uint64()
        capi.check(self.lib.vsrmc_test_table_export_import(self.h, window, new_log2, C.byref(n)))
        return n.value

    def table_log2(self):
        o = capi.Options()
        capi.check(self.lib.vsrmc_checker_options(self.h, C.byref(o)))
        return o.table_log2

    def check(self, model, what):
        """the dump against the model: content as a set of (fp, meta), the probing invariant; then every lookup path over the same table"""
        fps, metas = self.dump()
        none(sm.compare_dump(fps, metas, model, what + ": "))
        if model:
            keys = u64(sorted(model))
            found, ms = self.probe_lookup(keys)
            for i, f in enumerate(keys):
                need(found[i] == 1 and int(ms[i]) == model[int(f)],
                     "%s: probe_lookup of fp %016x: found %d meta %016x, model meta %016x" % (what, int(f), found[i], int(ms[i]), model[int(f)]))
        return fps, metas

    def close(self):
        self.mc.close()
        self.model.close()


def one_each(fps, level, seed=7, parents=None):
    """one candidate per fingerprint: (fp, key) rows and the model's table of them"""
    rng = np.random.default_rng([seed, level, len(fps)])
    rows = []
    for f in fps:
        par = int(parents[int(rng.integers(0, len(parents)))]) if parents is not None else int(rng.integers(1, 1 << 62))
        rows.append((int(f), sm.meta_make(level, int(rng.integers(0, 512)), par)))
    return np.array(rows, dtype=np.uint64).reshape(-1, 2)


def claim_and_check(t, model, entries, level, scheme, what, expect_err=0):
    """one launch of a claim scheme over `entries`; verdicts, ties and error against the model; -> the model's table afterwards"""
    batch = sm.batch_list(entries)
    ver, ctl = t.claim(entries, level, scheme)
    need(ctl["err"] == expect_err, "%s: control block error %d, expected %d" % (what, ctl["err"], expect_err))
    if scheme == 0:
        none(sm.check_exact_verdicts(model, batch, level, ver))
        need(ctl["ties"] == 0, "%s: the two-kernel scheme counted %d ties" % (what, ctl["ties"]))
        return sm.claim_exact(model, batch, level)
    none(sm.check_fused_verdicts(model, batch, level, ver, ctl["ties"]))
    return sm.claim_fused(model, batch, level)


def absent_of_home(log2, home, have, n, seed):
    have = {int(f) for f in have}
    return u64([f for f in sm.cluster(log2, home, n + len(have) // 50 + 4, seed=seed) if int(f) not in have][:n])


def edge_homes(S):
    return [0, 1, 2, 3, 4, S - 5, S - 4, S - 3, S - 2, S - 1]


# ---- 1. line and wrap geometry --------------------------------------------------------------------------------------------------------------------------
def geometry(scheme):
    for log2 in (8, 10):
        S = 1 << log2
        t = Table(log2)
        for home in edge_homes(S):
            what = "2^%d slots, home %d, scheme %d" % (log2, home, scheme)
            t.clear()
            fps = sm.cluster(log2, home, (3 * S) // 4, seed=11 + scheme)
            model = claim_and_check(t, {}, one_each(fps, 3), 3, scheme, what)
            d_fps, _ = t.check(model, what)
            occ = np.nonzero(d_fps)[0]
            need(len(occ) == len(fps) and set(int(j) for j in occ) == {(home + k) & (S - 1) for k in range(len(fps))},
                 "%s: the cluster does not occupy the %d slots from its home on" % (what, len(fps)))
            absent = absent_of_home(log2, home, fps, 40, seed=99)
            ask = np.concatenate([fps, absent, fps[:17]])
            for level, present in ((4, 1), (3, 0)):                       # "a state of a level below `level`": level 3 states are seen from level 4 only
                got = t.seen_batch(ask, level)
                exp = np.array(sm.seen_below(model, ask, level), dtype=np.uint8)
                bad = np.nonzero(got != exp)[0]
                need(len(bad) == 0, "%s: seen_batch(level %d) of fp %016x says %d, model %d" % (
                    what, level, int(ask[bad[0]]) if len(bad) else 0, got[bad[0]] if len(bad) else 0, exp[bad[0]] if len(bad) else 0))
                need(int(exp[:len(fps)].sum()) == present * len(fps), "model")
            found, ms = t.probe_lookup(absent)
            need(not found.any() and (ms == np.uint64(sm.META_EMPTY)).all(), "%s: probe_lookup found an absent fingerprint of the cluster's home" % what)
            for f in absent[:3]:
                need(t.lookup(int(f), 0, False)[0] == 0, "%s: lookup found absent fp %016x" % (what, int(f)))
        t.close()


# ---- 2. arbitration -----------------------------------------------------------------------------------------------------------------------------------
def arbitration_state(t, log2, scheme, wrap, seed=5, shrink=1):
    """level 5 from one batch, then a level-6 batch of duplicates that mixes new fingerprints, fingerprints of level 5 and (single-pass scheme) padding;
    -> the model's table"""
    S = 1 << log2
    rng = np.random.default_rng([seed, log2, scheme, int(wrap)])
    if wrap:
        old = sm.cluster(log2, S - 3, S // 4 // shrink, seed=seed)
        new = np.concatenate([sm.cluster(log2, S - 3, S // 4 // shrink, seed=seed + 1), sm.cluster(log2, S - 2, S // 8 // shrink, seed=seed + 2)])
        new = u64([f for f in new if int(f) not in {int(o) for o in old}])
    else:
        old = u64(sorted({int(v) | 1 for v in rng.integers(1, 1 << 63, size=S // 4, dtype=np.uint64)}))
        new = u64(sorted({int(v) & ~1 | 2 for v in rng.integers(1, 1 << 63, size=(3 * S) // 8, dtype=np.uint64)}))
    what = "arbitration, 2^%d slots, scheme %d%s" % (log2, scheme, ", wrapping cluster" if wrap else "")
    model = claim_and_check(t, {}, one_each(old, 5), 5, scheme, what + ", level 5")
    level5 = dict(model)
    mixed = np.concatenate([new, old[::2]])
    batch = sm.dup_batch(mixed, 6, seed=seed, parents=old, pad=37 if scheme == 1 else 0)
    need(len(batch) % 64 != 0 and len(batch) > 256, "model: the batch must span blocks and end inside a wave")
    model = claim_and_check(t, model, batch, 6, scheme, what + ", level 6")
    for f in old:
        need(model[int(f)] == level5[int(f)], "model")
    t.check(model, what)
    if scheme == 0:
        # the same level claimed again after its taken bits were cleared: a key EQUAL to the slot's meta word is not "beaten already" (table_claim), so
        # every state is granted exactly once more, the states of level 5 lose again, and the table ends as it was
        t.untake(6)
        again = claim_and_check(t, sm.untake(model, 6), batch[np.random.default_rng(seed).permutation(len(batch))], 6, 0, what + ", level 6 claimed again")
        need(again == model, "model: a level claimed twice")
        t.check(model, what + ", level 6 claimed again")
    return model


def arbitration(scheme):
    for wrap in (False, True):
        t = Table(10)
        arbitration_state(t, 10, scheme, wrap)
        t.close()


# ---- 3. probe bound -----------------------------------------------------------------------------------------------------------------------------------
def probe_bound(scheme):
    log2, home = 15, (1 << 15) - 6                                       # the run crosses the end of the table; home is slot 2 of its line: the shortest reach
    t = Table(log2)
    need(sm.probe_reach(home) == 8190 and min(sm.probe_reach(h) for h in range(4)) == 8190, "model")
    fps = sm.cluster(log2, home, 8000, seed=3)
    what = "probe bound, 8000 of one home, scheme %d" % scheme
    model = claim_and_check(t, {}, one_each(fps, 2), 2, scheme, what)
    t.check(model, what)
    # more than any probe reaches: ERR_TABLE_FULL, and nothing is lost that the error does not account for
    t.clear()
    n = 8192 + 64
    fps = sm.cluster(log2, home, n, seed=4)
    entries = one_each(fps, 2)
    ver, ctl = t.claim(entries, 2, scheme)
    what = "probe bound, %d of one home, scheme %d" % (n, scheme)
    need(ctl["err"] == sm.ERR_TABLE_FULL, "%s: control block error %d, expected ERR_TABLE_FULL" % (what, ctl["err"]))
    d_fps, d_metas = t.dump()
    none(sm.check_probing(d_fps, d_metas))
    got = sm.dump_content(d_fps, d_metas)
    reach = sm.probe_reach(home)
    need(len(got) == reach, "%s: %d fingerprints landed, the probe reaches %d slots" % (what, len(got), reach))
    occ = {int(j) for j in np.nonzero(d_fps)[0]}
    need(occ == {(home + k) & ((1 << log2) - 1) for k in range(reach)}, "%s: the occupied slots are not the %d slots from the home on" % (what, reach))
    want = {int(a): int(b) for a, b in entries}
    for i, (f, key) in enumerate(sm.batch_list(entries)):
        if f in got:
            exp = key | sm.META_TAKEN if scheme == 0 else key
            need(got[f] == exp and ver[i] == 1, "%s: fp %016x landed with meta %016x verdict %d, expected %016x and 1" % (what, f, got[f], ver[i], exp))
        else:
            need(ver[i] == 0, "%s: fp %016x is not in the table but won" % (what, f))     # dropped with the error raised, never as a winner
    need(set(got) <= set(want), "%s: a fingerprint nobody claimed is in the table" % what)
    landed = u64(sorted(got))
    found, ms = t.probe_lookup(landed)
    need(found.all() and all(int(ms[i]) == got[int(f)] for i, f in enumerate(landed)), "%s: probe_lookup misses a fingerprint of the dump" % what)
    for f in (landed[0], landed[len(landed) // 2], landed[-1]):
        fnd, ff, mm = t.lookup(int(f), 0, False)
        need(fnd == 1 and ff == int(f) and mm == got[int(f)], "%s: lookup of fp %016x" % (what, int(f)))
    lost = u64(sorted(set(want) - set(got)))
    need(len(lost) == n - reach, "model")
    found, _ = t.probe_lookup(lost)
    need(not found.any(), "%s: probe_lookup finds a fingerprint that is not in the dump" % what)
    need(not t.seen_batch(lost[:64], 3).any() and t.seen_batch(landed[-64:], 3).all(), "%s: seen_batch beyond / at the end of the run" % what)
    t.close()


# ---- 4. growth ----------------------------------------------------------------------------------------------------------------------------------------
def growth():
    for scheme in (0, 1):
        log2 = 10
        t = Table(log2)
        model = arbitration_state(t, log2, scheme, True)
        S = 1 << log2
        for extra, home in ((0, 1), (1, S - 2), (2, 3)):                  # clusters that two doublings split into four, two and one
            fps = u64([f for f in sm.cluster(log2, home, 60, extra_equal_bits=extra, seed=21) if int(f) not in model])
            model = claim_and_check(t, model, one_each(fps, 7 + extra), 7 + extra, scheme, "growth: cluster with %d equal bits" % extra)
            homes4 = {int(f) & (4 * S - 1) for f in fps}
            need(len(homes4) == 4 >> extra, "model: two doublings split the cluster with %d equal bits into %d" % (extra, len(homes4)))
        need(len(model) <= 0.85 * S, "model: load %f" % (len(model) / S))
        t.check(model, "growth, before")
        for step in (1, 2):
            t.grow()
            need(t.table_log2() == log2 + step and t.slots() == S << step, "growth: table_log2 %d, %d slots after %d doublings" % (t.table_log2(), t.slots(), step))
            t.check(model, "growth, scheme %d, 2^%d slots" % (scheme, log2 + step))
        t.close()


# ---- 5. export / import -------------------------------------------------------------------------------------------------------------------------------
def export_import():
    log2 = 10
    t = Table(log2)
    model = arbitration_state(t, log2, 0, True, shrink=2)                # taken bits included
    rng = np.random.default_rng(77)
    more = u64(sorted({int(v) for v in rng.integers(1, 1 << 63, size=60, dtype=np.uint64)} - set(model)))
    model = claim_and_check(t, model, one_each(more, 9), 9, 1, "export: level 9")
    for window in (64, 256, 1 << 20):
        for new_log2 in (log2 - 1, log2, log2 + 2):
            cur = t.table_log2()
            if new_log2 == cur - 1:
                need(len(model) <= 0.8 * (1 << new_log2), "model: %d entries are more than 0.8 of half the table" % len(model))
            n = t.export_import(window, new_log2)
            what = "export in windows of %d slots, import 2^%d -> 2^%d slots" % (window, cur, new_log2)
            need(n == len(model), "%s: the export counters add up to %d, the table held %d" % (what, n, len(model)))
            need(t.table_log2() == new_log2 and t.slots() == 1 << new_log2, what + ": size of the new table")
            t.check(model, what)
            if new_log2 != log2:
                n = t.export_import(window, log2)                         # back to 2^10 for the next case
                need(n == len(model), what + ": count on the way back")
                t.check(model, what + ", and back")
    t.close()


# ---- 6. untake and level checksum ---------------------------------------------------------------------------------------------------------------------
def untake_checksum():
    log2 = 10
    rng = np.random.default_rng(61)
    all_fps = u64(sorted({int(v) for v in rng.integers(1, 1 << 63, size=600, dtype=np.uint64)}))
    parts = {4: all_fps[:170], 5: np.concatenate([all_fps[170:399], sm.cluster(log2, (1 << log2) - 2, 40, seed=8)]), 6: all_fps[399:]}
    for min_level in (4, 5, 6, 7):
        t = Table(log2)
        model = {}
        for level, fps in parts.items():
            half = rng.permutation(len(fps))
            taken, plain = fps[half[:len(fps) // 2]], fps[half[len(fps) // 2:]]
            model = claim_and_check(t, model, one_each(taken, level), level, 0, "untake: level %d, taken" % level)      # two-kernel scheme: taken bit set
            model = claim_and_check(t, model, one_each(plain, level), level, 1, "untake: level %d, plain" % level)      # single-pass scheme: not set
        need(sum(m & 1 for m in model.values()) == sum(len(p) // 2 for p in parts.values()), "model")
        t.check(model, "untake, before")
        for level in (3, 4, 5, 6, 7):                                     # 3 and 7 are absent: all zero
            got, exp = t.level_checksum(level), sm.level_checksum(model, level)
            need(got == exp, "level checksum of level %d: (xor, sum, count) = %s, model %s" % (level, got, exp))
            fl = u64([f for f, m in model.items() if sm.meta_level(m) == level])
            if len(fl):
                npx = (int(np.bitwise_xor.reduce(fl)), int(np.add.reduce(fl, dtype=np.uint64)), len(fl))
                need(got == npx, "level checksum of level %d against numpy: %s, %s" % (level, got, npx))
            else:
                need(got == (0, 0, 0), "level checksum of the absent level %d: %s" % (level, got))
        t.untake(min_level)
        model = sm.untake(model, min_level)
        need(all((m & 1) == 0 for m in model.values() if sm.meta_level(m) >= min_level), "model")
        t.check(model, "untake(%d)" % min_level)
        t.close()


# ---- 7. walk ------------------------------------------------------------------------------------------------------------------------------------------
def walk():
    log2, depth = 10, 12
    S = 1 << log2
    t = Table(log2)
    model = {}
    fill = {}
    chains = {"ok": [], "ambiguous": [], "broken": []}
    # every level: a cluster that wraps (home S - 3); three chain states per level sit inside it, the rest is filler
    for level in range(1, depth + 1):
        fps = sm.cluster(log2, S - 3, 30, seed=100 + level)
        fill[level] = fps
        for k, name in enumerate(chains):
            chains[name].append(int(fps[5 + 7 * k]))
    rows = {}
    for level in range(1, depth + 1):
        rows[level] = []
        used = set()
        for name in chains:
            f = chains[name][level - 1]
            par = chains[name][level - 2] if level > 1 else 0
            rows[level].append((f, sm.meta_make(level, 17, par)))
            used.add(f)
        for f in fill[level]:
            if int(f) not in used:
                rows[level].append((int(f), sm.meta_make(level, 3, int(fill[level - 1][0]) if level > 1 else 0)))
    # decoys.  (a) a state of ANOTHER level with the low 45 bits of a parent of the good chain: ignored
    d_other = int(sm.same_low45(chains["ok"][5], 1, seed=1)[0])
    rows[9].append((d_other, sm.meta_make(9, 1, int(fill[8][1]))))
    # (b) a state of the SAME level with the low 45 bits of the ambiguous chain's level-4 state: status 2, level 4, two matches
    d_same = int(sm.same_low45(chains["ambiguous"][3], 1, seed=2)[0])
    rows[4].append((d_same, sm.meta_make(4, 1, int(fill[3][1]))))
    # (c) the broken chain's level-7 state is never inserted
    rows[7] = [r for r in rows[7] if r[0] != chains["broken"][6]]
    for level in range(1, depth + 1):
        model = claim_and_check(t, model, np.array(rows[level], dtype=np.uint64).reshape(-1, 2), level, level % 2, "walk: level %d" % level)
    t.check(model, "walk")
    for name, exp_status in (("ok", 0), ("ambiguous", 2 | (4 << 8) | (2 << 16)), ("broken", 1)):
        tip = chains[name][-1]
        m_status, m_fps = sm.walk(model, tip, depth)
        need(m_status == exp_status, "model: walk of the %s chain gives status %x" % (name, m_status))
        status, raw, rc, fps, msg = t.walk(tip, depth)
        need(status == exp_status, "walk of the %s chain: status %x, model %x" % (name, status, exp_status))
        if exp_status == 0:
            need(raw == m_fps == chains[name] and rc == 0 and fps == m_fps, "walk of the good chain: %s, model %s (walk_trace: %d)" % (raw, m_fps, rc))
        elif exp_status == 1:
            need(raw[0] == 0 and rc != 0, "walk of the broken chain: first entry %x, walk_trace returned %d" % (raw[0], rc))
        else:
            need(rc != 0 and "2 states of level 4" in msg, "walk of the ambiguous chain: walk_trace returned %d, '%s'" % (rc, msg))
    # a shorter walk from the middle of the good chain, and one at the wrong level
    status, raw, rc, fps, _ = t.walk(chains["ok"][6], 7)
    need(status == 0 and raw == chains["ok"][:7] and rc == 0, "walk from level 7")
    need(t.walk(chains["ok"][6], 8)[0] == 1, "walk from a state at the wrong level")
    # lookup in both modes on the same table
    for name in chains:
        for level in range(1, depth + 1):
            f = chains[name][level - 1]
            fnd, ff, mm = t.lookup(f, 0, False)
            if f in model:
                need((fnd, ff, mm) == (1, f, model[f]), "lookup of fp %016x: (%d, %016x, %016x), model meta %016x" % (f, fnd, ff, mm, model[f]))
            else:
                need(fnd == 0, "lookup finds the missing fp %016x" % f)
            match = sm.lookup_low_bits(model, f & sm.PFP_MASK, level)
            fnd, ff, mm = t.lookup(f & sm.PFP_MASK, level, True)
            need(fnd == len(match), "lookup by low bits of %012x at level %d: %d matches, model %d" % (f & sm.PFP_MASK, level, fnd, len(match)))
            if match:
                need(ff in match and mm == model[ff], "lookup by low bits of %012x at level %d: (%016x, %016x)" % (f & sm.PFP_MASK, level, ff, mm))
    need(t.lookup(d_other & sm.PFP_MASK, 6, True)[0] == 1 and t.lookup(d_other & sm.PFP_MASK, 9, True)[:2] == (1, d_other), "lookup by low bits: the decoy of another level")
    need(t.lookup(d_same & sm.PFP_MASK, 5, True)[0] == 0, "lookup by low bits at a level without a match")
    t.close()


# ---- 8. winner set ------------------------------------------------------------------------------------------------------------------------------------
class WSetDev:
    def __init__(self, log2):
        self.lib = capi.load()
        self.h = C.c_void_p()
        capi.check(self.lib.vsrmc_test_wset_create(0, log2, C.byref(self.h)))

    def dump(self):
        n = C.c_uint64()
        capi.check(self.lib.vsrmc_test_wset_dump(self.h, None, None, 0, C.byref(n)))
        fp = np.zeros(n.value, dtype=np.uint64)
        ep = np.zeros(n.value, dtype=np.uint32)
        capi.check(self.lib.vsrmc_test_wset_dump(self.h, _p(fp), _p(ep), n.value, C.byref(n)))
        return fp, ep

    def grow(self):
        capi.check(self.lib.vsrmc_test_wset_grow(self.h))

    def export_import(self, window, new_log2):
        n = C.c_uint64()
        capi.check(self.lib.vsrmc_test_wset_export_import(self.h, window, new_log2, C.byref(n)))
        return n.value

    def take(self, fps, level, epoch):
        f = u64(fps)
        out = np.zeros(len(f), dtype=np.uint8)
        capi.check(self.lib.vsrmc_test_wset_take(self.h, _p(f), len(f), level, epoch, _p(out)))
        return out

    def insert(self, mode, entries, cand_idx, verdict, level, nx_off=None, lvl_fp=None, pending_cap=0, with_set=True):
        e = u64(entries).reshape(-1, 2)
        ci = u64(cand_idx)
        v = np.ascontiguousarray(verdict, dtype=np.uint8)
        out = np.zeros(8, dtype=np.uint64)
        pend = np.zeros(2 * max(1, pending_cap), dtype=np.uint64)
        capi.check(self.lib.vsrmc_test_wset_insert(self.h if with_set else None, 0, mode, _p(e), _p(ci), _p(v), len(e), level,
                                                   _p(nx_off) if nx_off is not None else None, _p(lvl_fp) if lvl_fp is not None else None,
                                                   len(nx_off) if nx_off is not None else 0, _p(pend), pending_cap, _p(out)))
        names = ("err", "viol_fp", "viol_mask", "n_new", "fp_xor", "fp_sum", "max_bag", "n_pending")
        return dict(zip(names, (int(x) for x in out))), pend.reshape(-1, 2)

    def check(self, ws, what):
        fp, ep = self.dump()
        none(sm.check_probing(fp, None, home_of=sm.wset_home))
        got = {int(fp[j]): int(ep[j]) for j in np.nonzero(fp)[0]}
        exp = ws.words()
        for f in sorted(set(got) | set(exp)):
            need(got.get(f) == exp.get(f), "%s: winner set, fp %016x: epoch word %s, model %s" % (what, f, got.get(f), exp.get(f)))

    def close(self):
        self.lib.vsrmc_test_wset_destroy(self.h)


def take_rounds(w, ws, present, absent, levels, what):
    """epochs 1, 2, 2 again, 3 — a batch with duplicates and absent keys, per level of the set and at a wrong level"""
    rng = np.random.default_rng(len(present))
    for epoch, fresh in ((ws.next_epoch, True), (ws.next_epoch + 1, True), (ws.next_epoch + 1, False), (ws.next_epoch + 2, True)):
        for level in levels + [max(levels) + 1]:                           # the last one: nobody's level
            ask = np.concatenate([present, absent, present[rng.integers(0, len(present), size=len(present) // 2)], present[::3]])
            ask = ask[rng.permutation(len(ask))]
            need(len(ask) % 64 != 0, "model")
            got = w.take(ask, level, epoch)
            exp = ws.take_batch_counts(ask, level, epoch)
            for f in exp:
                trues = int(got[ask == np.uint64(f)].sum())
                need(trues == exp[f], "%s: take(fp %016x, level %d, epoch %d): %d lanes won, model %d" % (what, f, level, epoch, trues, exp[f]))
            n_true = sum(exp.values())
            if not fresh or level == max(levels) + 1:
                need(n_true == 0, "model: a repeated epoch / a wrong level takes nothing")
            else:
                need(n_true == sum(1 for f in set(int(x) for x in present) if ws.d[f][0] == level), "model: one take per present fingerprint of the level")
    ws.next_epoch += 3
    w.check(ws, what)


def winner_set():
    log2 = 8
    S = 1 << log2
    w = WSetDev(log2)
    ws = sm.WinnerSet()
    ws.next_epoch = 1
    levels = [6, 7]
    groups = {6: np.concatenate([sm.wset_cluster(log2, S - 2, 50, seed=1), sm.wset_cluster(log2, 0, 20, extra_equal_bits=2, seed=2)]),
              7: np.concatenate([sm.wset_cluster(log2, S - 2, 30, seed=3), sm.wset_cluster(log2, 3, 25, extra_equal_bits=1, seed=4)])}
    absent = np.concatenate([sm.wset_cluster(log2, S - 2, 20, seed=50), sm.wset_cluster(log2, 3, 9, seed=51)])
    rng = np.random.default_rng(12)
    # level 6 through k_apply_verdict, level 7 through k_count_verdict: winners, losers, padding, violators; n no multiple of 64
    for level, mode in ((6, 0), (7, 1)):
        winners = groups[level]
        losers = sm.wset_cluster(log2, S - 2, 45, seed=60 + level)
        rows, ver = [], []
        for f in winners:
            for _ in range(int(rng.integers(1, 3))):                      # a winner may be announced twice with the verdict 1 (two instances, one state: inserted once)
                rows.append(int(f)); ver.append(1)
        for f in losers:
            rows.append(int(f)); ver.append(0)
        rows += [0] * 21; ver += [1] * 21                                 # padding is skipped whatever its verdict byte says
        order = rng.permutation(len(rows))
        fps = u64([rows[i] for i in order]); ver = np.array([ver[i] for i in order], dtype=np.uint8)
        n = len(fps)
        need(n % 64 != 0 and n > 128, "model")
        entries = np.stack([fps, u64([sm.meta_make(level, int(a), 0) if f else 0 for f, a in zip(fps, rng.integers(0, 512, size=n))])], axis=1)
        bad = np.where(rng.integers(0, 5, size=n) == 0, rng.integers(1, 32, size=n), 0).astype(np.uint64)
        won = (fps != 0) & (ver == 1)
        if mode == 0:
            n_idx = n + 13
            idx = u64(rng.permutation(n_idx)[:n])
            nx_off = u64(rng.integers(1, 1 << 40, size=n_idx)); lvl_fp = u64(rng.integers(1, 1 << 63, size=n_idx))
            exp_off, exp_fp = nx_off.copy(), lvl_fp.copy()
            for i in range(n):
                if fps[i] != 0 and not ver[i]:
                    exp_off[idx[i]] = 0; exp_fp[idx[i]] = 0
            out, _ = w.insert(0, entries, idx | (bad << np.uint64(56)), ver, level, nx_off, lvl_fp)
            need(np.array_equal(nx_off, exp_off) and np.array_equal(lvl_fp, exp_fp), "k_apply_verdict: the withdrawn refs / fingerprints differ from the model")
            need((out["n_new"], out["n_pending"], out["max_bag"]) == (0, 0, 0), "k_apply_verdict wrote counters it does not own: %s" % out)
        else:
            bags = u64(rng.integers(0, 200, size=n))
            cap = 4
            out, pend = w.insert(1, entries, bags | (bad << np.uint64(56)), ver, level, pending_cap=cap)
            wf = fps[won]
            need(out["n_new"] == int(won.sum()) and out["fp_xor"] == int(np.bitwise_xor.reduce(wf)) and out["fp_sum"] == int(np.add.reduce(wf, dtype=np.uint64))
                 and out["max_bag"] == int(bags[won].max()), "k_count_verdict: n_new / fp_xor / fp_sum / max_bag %s differ from the model" % out)
            viol = won & (bad != 0)
            need(out["n_pending"] == int(viol.sum()) and out["n_pending"] > cap, "k_count_verdict: %d pending, model %d" % (out["n_pending"], int(viol.sum())))
            pairs = {(int(a), int(b)) for a, b in entries[viol]}
            need(all((int(a), int(b)) in pairs for a, b in pend[:cap]), "k_count_verdict: a pending entry that is no violating winner")
        viol = won & (bad != 0)
        need(out["err"] == 0, "winner set: error %d" % out["err"])
        need(out["viol_fp"] == (int(fps[viol].min()) if viol.any() else sm.M64) and out["viol_mask"] == int(np.bitwise_or.reduce(bad[viol])),
             "viol_fp / viol_mask (%016x, %x) differ from the model" % (out["viol_fp"], out["viol_mask"]))
        for f in winners:
            ws.insert(int(f), level)
        w.check(ws, "after the level-%d verdicts" % level)
    # without a set the two kernels do the same bookkeeping and touch no set
    e1 = np.array([[int(groups[6][0]), sm.meta_make(8, 1, 0)]], dtype=np.uint64)
    out, _ = w.insert(1, e1, u64([5]), np.array([1], dtype=np.uint8), 8, with_set=False)
    need(out["n_new"] == 1 and out["max_bag"] == 5, "k_count_verdict without a set")
    w.check(ws, "after a launch without a set")
    present = np.concatenate([groups[6], groups[7]])
    take_rounds(w, ws, present, absent, levels, "2^8 slots")
    w.grow()
    take_rounds(w, ws, present, absent, levels, "after one doubling")
    w.grow()
    take_rounds(w, ws, present, absent, levels, "after two doublings")
    for window, new_log2 in ((64, 8), (100, 9), (1 << 20, 8)):
        n = w.export_import(window, new_log2)
        need(n == len(ws.d), "winner set: export counted %d, the set holds %d" % (n, len(ws.d)))
        ws.export_import()
        ws.next_epoch = 1                                                 # the descent counter starts over, like the recovered checker's
        w.check(ws, "after export / import")
        take_rounds(w, ws, present, absent, levels, "after export (windows of %d) / import into 2^%d" % (window, new_log2))
    w.close()


# ---- 9. partition -------------------------------------------------------------------------------------------------------------------------------------
def partition():
    lib = capi.load()
    rng = np.random.default_rng(9)
    for world in (2, 3, 8):
        for n in (1, 63, 1000 + world):
            fps = u64(rng.integers(1, 1 << 63, size=n, dtype=np.uint64)) | (u64(rng.integers(0, 2, size=n)) << np.uint64(63))
            off = u64(rng.integers(1, 1 << 40, size=n))
            if n > 1:
                off[rng.integers(0, n, size=n // 7)] = 0                   # refs that are invalid already
            for rank in range(world):
                o, f = off.copy(), fps.copy()
                kept = C.c_uint64()
                capi.check(lib.vsrmc_test_table_partition(0, _p(o), _p(f), n, rank, world, C.byref(kept)))
                mine = np.array([off[i] != 0 and sm.owner_of(int(fps[i]), world) == rank for i in range(n)])
                need(kept.value == int(mine.sum()), "partition, world %d rank %d, n %d: kept %d, model %d" % (world, rank, n, kept.value, int(mine.sum())))
                exp_o = np.where(mine | (off == 0), off, 0).astype(np.uint64)
                exp_f = np.where(mine | (off == 0), fps, 0).astype(np.uint64)     # an invalid ref keeps whatever fingerprint word it had
                need(np.array_equal(o, exp_o) and np.array_equal(f, exp_f), "partition, world %d rank %d, n %d: the surviving indices differ from the model" % (world, rank, n))


COMMANDS = {
    "geometry_exact": lambda: geometry(0), "geometry_fused": lambda: geometry(1),
    "arbitration_exact": lambda: arbitration(0), "arbitration_fused": lambda: arbitration(1),
    "probe_bound_exact": lambda: probe_bound(0), "probe_bound_fused": lambda: probe_bound(1),
    "growth": growth, "export_import": export_import, "untake_checksum": untake_checksum, "walk": walk,
    "winner_set": winner_set, "partition": partition,
}

if __name__ == "__main__":
    try:
        COMMANDS[sys.argv[1]]()
    except Mismatch as e:
        print("MISMATCH %s: %s" % (sys.argv[1], e))
        sys.exit(1)
    print("OK", sys.argv[1])
