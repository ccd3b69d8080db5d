"""A host model of the seen-set (csrc/vsr_kernels.hpp: probe_insert / probe_lookup / table_claim / table_claim_fused and the kernels around them), of the
winner set of a sharded deep search and of k_partition — pure Python / numpy, no GPU, and NO PROBING: it restates WHAT the tables must hold, not how
the kernels get there.  tests/seen_set_worker.py drives the real kernels against it; tests/test_seen_set_model.py checks the model against itself.

A table is a dict {fingerprint: meta word} of Python ints.  The meta word is written from the layout comment in csrc/vsr_model.hpp:
    level(9) << 55 | canonical auxkey(9) << 46 | low 45 bits of the parent's fingerprint << 1 | taken(1);   smaller = wins the slot
"""
import numpy as np

M64 = (1 << 64) - 1
META_EMPTY = M64
META_TAKEN = 1
PFP_MASK = (1 << 45) - 1
ERR_TABLE_FULL = 20
PROBE_LINES = 2048          # probe_insert / probe_lookup give up after this many 64-byte lines beyond the home slot


def meta_make(level, auxkey, parent_fp):
    assert 0 <= level < 512 and 0 <= auxkey < 512
    return (level << 55) | (auxkey << 46) | ((parent_fp & PFP_MASK) << 1)


def meta_level(m):
    return m >> 55


def meta_auxkey(m):
    return (m >> 46) & 511


def meta_pfp(m):
    return (m >> 1) & PFP_MASK


def owner_of(fp, world):
    return ((fp >> 40) & 0xFFFFFF) % world


def probe_reach(home):
    """Slots probe_insert inspects before it reports a full table: the home slot, the rest of the line the NEXT slot lies in, 2047 more lines."""
    return 1 + (4 - (home + 1) % 4) + (PROBE_LINES - 1) * 4


# ---- claims ---------------------------------------------------------------------------------------------------------------------------------------
def _groups(batch):
    g = {}
    for fp, key in batch:
        if fp != 0:
            g.setdefault(fp, []).append(key)
    return g


def claim_exact(table, batch, level):
    """k_claim_batch + k_verdict over one batch of (fp, key): the table afterwards.  A fingerprint of an earlier level keeps its meta word; otherwise the
    slot ends at the smallest key, taken (a same-level meta word already there takes part in the minimum)."""
    out = dict(table)
    for fp, keys in _groups(batch).items():
        old = out.get(fp)
        if old is not None and meta_level(old) < level:
            continue
        best = min(keys)
        if old is not None:
            best = min(best, old & ~META_TAKEN)
        out[fp] = best | META_TAKEN
    return out


def check_exact_verdicts(table, batch, level, verdict):
    """None, or what is wrong with the verdict bytes of the two-kernel scheme over a batch claimed into `table` (the table BEFORE the batch).  A
    fingerprint of the batch is new, of an earlier level, or of this level with its taken bit cleared (table_claim: only a SMALLER key of this level
    beats a candidate — an equal one does not, so a level claimed again after k_table_untake grants every state once more)."""
    won = {}
    for i, (fp, key) in enumerate(batch):
        if verdict[i] not in (0, 1):
            return "candidate %d (fp %016x): verdict byte %d" % (i, fp, verdict[i])
        if verdict[i]:
            won.setdefault(fp, []).append(key)
    for fp, keys in _groups(batch).items():
        best = min(keys)
        if fp in table:
            m = table[fp]
            if meta_level(m) > level or (meta_level(m) == level and m & META_TAKEN):
                return "fp %016x: the model's caller claimed a level that is taken already" % fp
            if meta_level(m) < level or m < best:
                if fp in won:
                    return "fp %016x of level %d (meta %016x) won again at level %d" % (fp, meta_level(m), m, level)
                continue
            # a state of THIS level whose taken bit was cleared (k_table_untake) and whose key is claimed again: a key equal to the slot's is not beaten
        w = won.get(fp, [])
        if len(w) != 1:
            return "fp %016x: %d winners among %d candidates" % (fp, len(w), len(keys))
        if w[0] != best:
            return "fp %016x: winner key %016x, smallest key %016x" % (fp, w[0], best)
    return None


def claim_fused(table, batch, level):
    """k_claim_batch_fused: the smallest key, no taken bit; fp == 0 leaves nothing behind."""
    out = dict(table)
    for fp, keys in _groups(batch).items():
        old = out.get(fp)
        if old is not None and meta_level(old) < level:
            continue
        best = min(keys)
        if old is not None:
            best = min(best, old)
        out[fp] = best
    return out


def fused_ties_expected(table, batch):
    """ties > 0 exactly when a NEW fingerprint has candidates with different auxkeys"""
    return any(fp not in table and len({meta_auxkey(k) for k in keys}) > 1 for fp, keys in _groups(batch).items())


def check_fused_verdicts(table, batch, level, verdict, ties):
    won = {}
    for i, (fp, key) in enumerate(batch):
        if verdict[i] not in (0, 1):
            return "candidate %d (fp %016x): verdict byte %d" % (i, fp, verdict[i])
        if verdict[i]:
            if fp == 0:
                return "candidate %d: padding (fp 0) won" % i
            won[fp] = won.get(fp, 0) + 1
    for fp, keys in _groups(batch).items():
        if fp in table:
            if meta_level(table[fp]) >= level:
                return "fp %016x: the model's caller claimed a level twice" % fp
            if fp in won:
                return "fp %016x of level %d won again at level %d" % (fp, meta_level(table[fp]), level)
        elif won.get(fp, 0) != 1:
            return "fp %016x: %d winners among %d candidates" % (fp, won.get(fp, 0), len(keys))
    if (ties > 0) != fused_ties_expected(table, batch):
        return "ties = %d, but candidates of one new fingerprint with different auxkeys: %s" % (ties, fused_ties_expected(table, batch))
    return None


# ---- the raw slot array ---------------------------------------------------------------------------------------------------------------------------
def dump_content(fps, metas):
    """{fp: meta} of a raw dump (two uint64 arrays, one entry per slot); a doubled fingerprint is kept out for check_probing to name"""
    occ = np.nonzero(fps)[0]
    return {int(fps[j]): int(metas[j]) for j in occ}


def check_probing(fps, metas=None, home_of=None):
    """The linear-probing invariant find_exact / find_by_low_bits rely on: every occupied slot is reachable from its home slot (fp & mask, or home_of(fp,
    mask)) without passing an empty slot, and no fingerprint occurs twice.  None, or the first violation."""
    fps = np.asarray(fps, dtype=np.uint64)
    S = len(fps)
    assert S and S & (S - 1) == 0
    mask = S - 1
    occ = np.nonzero(fps)[0]
    vals = fps[occ]
    u, first, cnt = np.unique(vals, return_index=True, return_counts=True)
    if (cnt > 1).any():
        f = int(u[np.argmax(cnt > 1)])
        slots = [int(j) for j in occ[vals == np.uint64(f)]]
        return "fp %016x occurs %d times: slots %s" % (f, len(slots), slots)
    empty_before = np.concatenate([[0], np.cumsum(np.concatenate([fps, fps]) == 0)])     # empties among the first k slots of the doubled array
    for j in occ:
        f = int(fps[j])
        h = home_of(f, mask) if home_of else f & mask
        d = (int(j) - h) & mask
        if empty_before[h + d] - empty_before[h] != 0:
            m = int(metas[j]) if metas is not None else 0
            return "fp %016x in slot %d (meta %016x) is cut off from its home slot %d by an empty slot" % (f, int(j), m, h)
    return None


def compare_dump(fps, metas, table, what=""):
    """None, or the first difference between a raw dump and the model's table (content as a set of (fp, meta), then the probing invariant)."""
    bad = check_probing(fps, metas)
    if bad:
        return what + bad
    got = dump_content(fps, metas)
    slot_of = {int(fps[j]): int(j) for j in np.nonzero(fps)[0]}
    for fp in sorted(set(got) | set(table)):
        a, b = got.get(fp), table.get(fp)
        if a != b:
            return what + "fp %016x slot %s: table holds meta %s, model %s" % (
                fp, slot_of.get(fp, "-"), "%016x" % a if a is not None else "nothing", "%016x" % b if b is not None else "nothing")
    return None


# ---- other restatements ---------------------------------------------------------------------------------------------------------------------------
def level_checksum(table, level):
    x = s = n = 0
    for fp, m in table.items():
        if meta_level(m) == level:
            x ^= fp
            s = (s + fp) & M64
            n += 1
    return x, s, n


def untake(table, min_level):
    return {fp: (m & ~META_TAKEN if (m & META_TAKEN) and m != META_EMPTY and meta_level(m) >= min_level else m) for fp, m in table.items()}


def seen_below(table, fps, level):
    return [1 if (int(f) in table and meta_level(table[int(f)]) < level) else 0 for f in fps]


def lookup_low_bits(table, pfp, level):
    """the states of `level` whose fingerprints end in the 45 bits `pfp`"""
    return sorted(f for f, m in table.items() if f & PFP_MASK == pfp & PFP_MASK and meta_level(m) == level)


def walk(table, fp, level):
    """The backwards walk over parent bits (k_trace_walk): (status, fps).  status 0: fps[l - 1] = the path's level-l state; 1: broken chain;
    2 | l << 8 | matches << 16: the pointer of the path's level-(l + 1) state is ambiguous."""
    fps = [0] * level
    cur = fp if fp in table else None
    for l in range(level, 0, -1):
        if cur is None or meta_level(table[cur]) != l:
            return 1, None
        fps[l - 1] = cur
        if l > 1:
            match = lookup_low_bits(table, meta_pfp(table[cur]), l - 1)
            if len(match) > 1:
                return 2 | ((l - 1) << 8) | (len(match) << 16), None
            cur = match[0] if match else None
    return 0, fps


def wset_home(fp, mask):
    return (fp >> 13) & mask


class WinnerSet:
    """{fp: (level, last_epoch)}: take(fp, level, epoch) is true once per (fp, epoch), only at the stored level and only for a later epoch"""

    def __init__(self):
        self.d = {}
        self.next_epoch = 1        # (the caller's descent counter)

    def insert(self, fp, level):
        self.d.setdefault(fp, (level, 0))

    def take(self, fp, level, epoch):
        e = self.d.get(fp)
        if e is None or e[0] != level or e[1] >= epoch:
            return False
        self.d[fp] = (level, epoch)
        return True

    def take_batch_counts(self, fps, level, epoch):
        """{fp: how many lanes of a batch must see `true`} (1 or 0 each), the set updated"""
        out = {}
        for f in fps:
            f = int(f)
            if f not in out:
                out[f] = 1 if self.take(f, level, epoch) else 0
        return out

    def export_import(self):
        self.d = {fp: (lv, 0) for fp, (lv, _e) in self.d.items()}

    def words(self):
        """{fp: epoch word} as the device keeps it: level(9) << 23 | last epoch"""
        return {fp: (lv << 23) | ep for fp, (lv, ep) in self.d.items()}


# ---- adversarial keys: seeded, deterministic ----------------------------------------------------------------------------------------------------------
def _distinct_high(rng, n, bits, forbid_zero):
    assert bits >= 1 and n <= (1 << min(bits, 62)) - (1 if forbid_zero else 0)
    seen, out = set(), []
    while len(out) < n:
        for v in rng.integers(0, 1 << min(bits, 63), size=2 * (n - len(out)) + 8, dtype=np.uint64):
            v = int(v) & ((1 << bits) - 1)
            if v in seen or (forbid_zero and v == 0):
                continue
            seen.add(v)
            out.append(v)
            if len(out) == n:
                break
    return out


def cluster(log2_slots, home, n, extra_equal_bits=0, seed=1):
    """n distinct non-zero fingerprints with fp & mask == home that also agree in the `extra_equal_bits` bits above the index (so that many doublings of
    the table do not split them)"""
    rng = np.random.default_rng([seed, log2_slots, home, n, extra_equal_bits])
    low = log2_slots + extra_equal_bits
    extra = int(rng.integers(0, 1 << extra_equal_bits)) if extra_equal_bits else 0
    base = (extra << log2_slots) | home
    return np.array([(h << low) | base for h in _distinct_high(rng, n, 64 - low, base == 0)], dtype=np.uint64)


def wset_cluster(log2_slots, home, n, extra_equal_bits=0, seed=1):
    """the same for the winner set, whose home slot is (fp >> 13) & mask"""
    rng = np.random.default_rng([seed, log2_slots, home, n, extra_equal_bits, 13])
    low = 13 + log2_slots + extra_equal_bits
    extra = int(rng.integers(0, 1 << extra_equal_bits)) if extra_equal_bits else 0
    base = ((extra << log2_slots) | home) << 13
    highs = _distinct_high(rng, n, 64 - low, True)
    lows = rng.integers(0, 1 << 13, size=n)
    return np.array([(h << low) | base | int(l) for h, l in zip(highs, lows)], dtype=np.uint64)


def same_low45(fp, k, seed=1):
    """k distinct fingerprints, none of them fp, that agree with fp in the low 45 bits"""
    rng = np.random.default_rng([seed, int(fp) & 0xFFFFFFFF, k])
    highs = [h for h in _distinct_high(rng, k + 1, 19, False) if h != int(fp) >> 45][:k]
    return np.array([(h << 45) | (int(fp) & PFP_MASK) for h in highs], dtype=np.uint64)


def dup_batch(fps, level, seed=1, parents=None, pad=0):
    """A shuffled batch of (fp, key): each fingerprint 1 - 7 times; the keys of one fingerprint differ in the auxkey, in the parent bits, or not at all
    (bit-identical candidates) — the kind cycles with the fingerprint's position, the multiplicity is drawn.  `pad` entries (0, 0) are mixed in.
    -> uint64 array of shape (n, 2)"""
    rng = np.random.default_rng([seed, level, len(fps), pad])
    rows = []
    for i, fp in enumerate(fps):
        k = int(rng.integers(1, 8))
        kind = i % 3
        aux = int(rng.integers(0, 512 - 8))
        par = int(parents[int(rng.integers(0, len(parents)))]) if parents is not None and len(parents) else int(rng.integers(1, 1 << 62))
        for j in range(k):
            if kind == 0:
                key = meta_make(level, aux + j, par)
            elif kind == 1:
                key = meta_make(level, aux, par + j)
            else:
                key = meta_make(level, aux, par)
            rows.append((int(fp), key))
    rows += [(0, 0)] * pad
    order = rng.permutation(len(rows))
    return np.array([rows[i] for i in order], dtype=np.uint64).reshape(-1, 2)


def batch_list(entries):
    return [(int(a), int(b)) for a, b in np.asarray(entries, dtype=np.uint64).reshape(-1, 2)]
