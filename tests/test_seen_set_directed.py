"""Directed tests of the seen-set kernels against the host model of tests/seen_set_model.py.

A search hands the seen-set uniform fingerprints at a load below 0.85, so whole-search parity only samples the easy middle of probe_insert /
probe_lookup / table_claim / table_claim_fused and of the kernels around them.  Here the keys are built to hit the edges — probe runs that start at
every slot of a 64-byte line, that cross the end of the table, that are thousands of slots long, several candidates of one fingerprint in one launch,
candidates that meet a state of an earlier level — and every test ends by comparing the raw slot array with the model: the content as a set of
(fingerprint, meta word), and the linear-probing invariant find_exact / find_by_low_bits rely on.

Tests 1 - 9 run tests/seen_set_worker.py in a child process that loads libvsrmc_hooks.so (the hooks of csrc/host_test_table.hpp launch the product
kernels one at a time); test 10 drives the stand-alone FPSet through the public API of the product library."""
import os
import subprocess
import sys

import numpy as np
import pytest

import seen_set_model as sm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(name):
    hooks = os.path.join(ROOT, "vsr_tlaplus_amd", "libvsrmc_hooks.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "seen_set_worker.py"), name], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, VSRMC_LIB=hooks))
    assert r.returncode == 0 and ("OK " + name) in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("scheme", ["exact", "fused"])
def test_line_and_wrap_geometry(scheme):
    """1. Clusters of 0.75 S fingerprints of one home, for the homes 0 .. 4 and S - 5 .. S - 1 (every start inside a line, runs that cross the end of
    the table), through k_claim_batch + k_verdict / k_claim_batch_fused; vsrmc_checker_seen_batch, probe_lookup and lookup afterwards, absent
    fingerprints of the same home included."""
    worker("geometry_" + scheme)


@pytest.mark.parametrize("scheme", ["exact", "fused"])
def test_arbitration(scheme):
    """2. A level-6 batch with every fingerprint 1 - 7 times (keys that differ in the auxkey, in the parent bits, or not at all) over a table that holds
    level 5: new fingerprints, fingerprints of level 5 (they lose, meta word untouched), padding (single-pass scheme: only its chunks have any).
    Two-kernel scheme: the smallest key wins, exactly one verdict per state also among bit-identical candidates, the taken bit is set.  Single-pass
    scheme: one verdict per new state, the smallest meta word, ties > 0 exactly when a new fingerprint has candidates with different auxkeys.  Uniform
    keys, then a cluster that wraps."""
    worker("arbitration_" + scheme)


@pytest.mark.parametrize("scheme", ["exact", "fused"])
def test_probe_bound(scheme):
    """3. 2^15 slots, one home (slot 2 of the line before the table's last: the shortest reach, and the run wraps).  8000 fingerprints land without an
    error (probe_insert reaches 1 + 2048 * 4 - 3 = 8190 slots at the least); 8192 + 64 raise ERR_TABLE_FULL, exactly the probe's reach of them
    land — each found by every lookup, each a winner — and every other one has verdict 0: nothing is dropped that the error does not account for."""
    worker("probe_bound_" + scheme)


def test_growth():
    """4. The state of test 2 (taken bits included) plus clusters that agree in 0, 1 and 2 bits above the index, through table_grow twice: the content
    identical, the invariant at each size, table_log2 advanced."""
    worker("growth")


def test_export_import():
    """5. k_table_export in windows of 64 and 256 slots and of the whole table, k_table_import into half the slots (load <= 0.8), the same and four
    times as many: the content identical, the count equal to the export counters."""
    worker("export_import")


def test_untake_and_level_checksum():
    """6. Three levels, taken bits on a random half: k_table_untake(min_level) for each level and one beyond; k_table_level_checksum of each level
    and of two absent ones against the model and numpy (xor, sum mod 2^64, count)."""
    worker("untake_checksum")


def test_walk():
    """7. k_trace_walk / walk_trace over chains of 12 levels whose states sit inside clusters that wrap: a decoy of another level with a parent's 45 low
    bits (ignored), one of the same level (status 2, that level, 2 matches), a chain with a missing state (status 1); table_lookup in both modes."""
    worker("walk")


def test_winner_set():
    """8. The winner set, clustered by its own home bits ((fp >> 13) & mask), wrap included: filled by k_apply_verdict and k_count_verdict (their other
    outputs against the model, n no multiple of 64); wset_take on batches with duplicates and absent keys at epochs 1, 2, 2 again and 3 — exactly one
    true per present fingerprint and new epoch, none on the repeat, none at a wrong level; the same after k_wset_rehash and after k_wset_export /
    k_wset_import (level kept, epoch restarted)."""
    worker("winner_set")


def test_partition():
    """9. k_partition for worlds of 2, 3 and 8 ranks, n no multiple of 64, invalid refs inside: kept count and surviving indices against owner_of."""
    worker("partition")


# ---- 10. the stand-alone FPSet (k_fpset_put / k_fpset_contains) with the same keys, through the public API of the product library -----------------------
@pytest.fixture(scope="module")
def vt():
    import vsr_tlaplus_amd as vt
    assert vt.load().vsrmc_device_count() >= 1, "no HIP device visible"
    return vt


@pytest.mark.parametrize("log2", [4, 8])
def test_fpset_clusters_wrap_and_the_exactly_full_table(vt, log2):
    S = 1 << log2
    for home in sorted({0, 1, 3, S - 4, S - 2, S - 1}):
        s = vt.FPSet(log2_slots=log2)
        fps = sm.cluster(log2, home, S + 9, seed=31)
        inside, beyond = fps[:S], fps[S:]
        first = inside[:(3 * S) // 4]
        assert not s.put_block(first).any() and s.size() == len(first)
        assert s.contains_block(first).all() and not s.contains_block(inside[len(first):]).any()
        # a batch with the rest, every key twice and some that are in already: one "new" per new key
        rest = inside[len(first):]
        was = s.put_block(np.concatenate([rest, first[:5], rest]))
        assert int((was == 0).sum()) == len(rest) and was[len(rest):len(rest) + 5].all()
        for f in rest:
            assert int((was[np.concatenate([rest, first[:5], rest]) == f] == 0).sum()) == 1
        assert s.size() == S                                        # filled to exactly S entries, no error
        assert s.contains_block(inside).all()
        assert not s.contains_block(beyond).any()                  # an absent key on the full table: false, and the scan ends
        assert s.put_block(inside).all() and s.size() == S          # present keys can still be put
        with pytest.raises(vt.VsrmcError):
            s.put(int(beyond[0]))                                   # the S + 1-th distinct key
        assert s.size() == S                                        # (the error is sticky: the handle reports it from here on, like a TLC FPSet that ran full)
        s.close()
