"""Child process of test_deep_action_constraint_gpu.py::test_forced_violations_in_a_child.  Runs with VSRMC_LIB = libvsrmc_hooks.so: the test hook
VSRMC_TEST_FORCE_BAD=<hex fingerprint>:<mask>, read when a model is built, makes one chosen state fail an invariant, so that the gated passes beyond the
record buffers have a violator to report (no reachable state of these small spaces violates anything).  QuietClient on (2,1,{v1,v2},2):
  (a) a RESCUED reference state of level 11, inserted by the record-less first pass from base 10: reported at that level, its behaviour takes permitted steps only
  (b) a reference state of level 12, the probed level of the descent that inserts level 11 from base 9: reported by the probe, the last step permitted
  (c) a blocked target of the step out of level 10 that never enters the model: no violation anywhere, counted in blocked_violating of level 11's passes,
      blocked_viol_min_fp one of its parents
  (d) every state of a stored level that overflows a tiny record buffer, one run each: the adopted level reports it, written or not."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import action_constraint_reference as ar                       # noqa: E402
import test_deep_action_constraint_gpu as T                    # noqa: E402
import vsr_tlaplus_amd as vt                                   # noqa: E402

KEY = "quiet-2122"
MASK = 1


def checker(bad_fp, base):
    os.environ["VSRMC_TEST_FORCE_BAD"] = "%x:%d" % (bad_fp, MASK)
    m = vt.Model.from_constants(R=2, C_=1, n=2, L=2)
    mc = vt.ModelChecker(m, device=0, **T.SIZES)
    mc.action_constrain(m.compile_step_predicates(ar.TEXTS["QuietClient"]), deep=True)
    for _ in range(base - 1):
        d = mc.step()
        assert d["viol_mask"] == 0, d["level"]
    assert mc.level == base
    return mc


def main():
    assert getattr(vt.load(), "vsrmc_test_checker_seed_records", None) is not None, "run me with VSRMC_LIB = libvsrmc_hooks.so"
    ref = ar.constrained_bfs("first", 2, 1, 2, 2, ar.quiet_client)
    # (a) the first pass, insert mode
    fp = min(ref.levels[10].rescued)
    mc = checker(fp, 10)
    a, p = mc.deepen()
    assert p is None and (a["level"], a["n_new"], a["viol_mask"], a["viol_fp"]) == (11, len(ref.levels[10].new), MASK, fp), a
    tr = mc.probe_trace()
    assert len(tr) == 11
    T._check_trace(tr, KEY, fp)
    assert mc.violation["level"] == 11 and mc.violation["fp"] == fp
    mc.close()
    print("a OK %016x" % fp)
    # (b) the probed level
    fp = min(ref.levels[11].new)
    mc = checker(fp, 9)
    a, p = mc.deepen()
    assert a["viol_mask"] == 0
    a, p = mc.deepen()
    assert (a["level"], a["viol_mask"]) == (11, 0) and p is not None
    assert (p["level"], p["viol_mask"], p["viol_fp"]) == (12, MASK, fp), p
    assert [int(f) for f in mc.probe_violators()] == [fp]
    tr = mc.probe_trace()
    assert len(tr) == 12
    T._check_trace(tr, KEY, fp)                                  # every step permitted, the last one — into the violator — included
    mc.close()
    print("b OK %016x" % fp)
    # (c) a blocked target that never enters the model
    never = T._never_entering(KEY, ref, 10)
    assert never
    fp = min(never)
    mc = checker(fp, 9)
    a, p = mc.deepen()
    assert a["viol_mask"] == 0
    a, p = mc.deepen()                                           # the descent that inserts level 11: the step out of level 10 generates the target, blocked
    assert (a["level"], a["viol_mask"]) == (11, 0) and (p is None or p["viol_mask"] == 0)
    di = mc.action_constraint_deep_results(11)
    assert di["blocked_violating"] >= 1 and di["blocked_viol_mask"] & MASK and di["blocked_viol_min_fp"] in never[fp], di
    while a["n_new"]:
        a, p = mc.deepen()
        assert a["viol_mask"] == 0 and (p is None or p["viol_mask"] == 0)
    assert mc.violation is None and (mc.depth, mc.distinct) == (27, 1510)
    assert mc.lookup(fp) is None
    mc.close()
    print("c OK %016x" % fp)
    # (d) a stored level that overflows its record buffer and is adopted has been checked WHOLE: record buffers of 512 words (256 usable) hold the first
    #     levels; the step into level `base + 1` overflows.  Which records were written nobody knows, so EVERY state of that level is forced in turn, in a run of
    #     its own: the level's records take more words than the buffer has, so at least one of these runs has its violator in a record that was not written.
    tiny = dict(T.SIZES, frontier_words=512, frontier_states=2048)
    os.environ.pop("VSRMC_TEST_FORCE_BAD", None)
    m = vt.Model.from_constants(R=2, C_=1, n=2, L=2)
    mc = vt.ModelChecker(m, device=0, **T.SIZES)
    mc.action_constrain(m.compile_step_predicates(ar.TEXTS["QuietClient"]))
    words = [0, 0] + [mc.step()["record_words"] for _ in range(8)]          # words[L]: the records of level L of the constrained search
    mc.close()
    mc = vt.ModelChecker(m, device=0, **tiny)
    mc.action_constrain(m.compile_step_predicates(ar.TEXTS["QuietClient"]), deep=True)
    try:
        while True:
            mc.step()
    except vt.VsrmcError:
        base = mc.level
    mc.close()
    level = ref.levels[base]                                       # level base + 1
    assert 3 <= base <= 7 and words[base + 1] > 256 and len(level.new) >= 6, (base, words)
    for fp in sorted(level.new):
        os.environ["VSRMC_TEST_FORCE_BAD"] = "%x:%d" % (fp, MASK)
        m = vt.Model.from_constants(R=2, C_=1, n=2, L=2)
        mc = vt.ModelChecker(m, device=0, **tiny)
        mc.action_constrain(m.compile_step_predicates(ar.TEXTS["QuietClient"]), deep=True)
        for _ in range(base - 1):
            mc.step()
        try:
            mc.step()
            raise AssertionError("the step into level %d fitted 256 words" % (base + 1))
        except vt.VsrmcError:
            pass
        kind, d, p = mc.advance()
        assert kind == "deep" and (d["level"], d["n_new"], d["viol_mask"], d["viol_fp"]) == (base + 1, len(level.new), MASK, fp), (fp, d)
        tr = mc.probe_trace()
        assert len(tr) == base + 1
        T._check_trace(tr, KEY, fp)
        mc.close()
    print("d OK: level %d, %d states, %d words of records against 256" % (base + 1, len(level.new), words[base + 1]))
    print("ALL OK")


if __name__ == "__main__":
    main()
