"""Child process of tests/test_model_invariants_gpu.py: the REPORTING path of the two analysis models on a seeded level (TEST INFRASTRUCTURE).

Runs with VSRMC_LIB = libvsrmc_hooks.so.  The seeds are the clean parents of class E of tests/invariant_mutants.py — states that violate
nothing and in which some enabled action makes a violation — put in as level 1 of a second-model / third-model checker
(ModelChecker.seed_records, csrc/host_test_seed.hpp: model-generic).  One step must then report, every figure from the C++ oracle alone
(tests/deep_seeded_worker.py Case / check_level, parameterised over the oracle module):

    generated, n_new, act_generated                  viol_mask = the or of the new states' verdicts
    viol_fp   = the smallest violating new fingerprint   trace = [seed, state] with the oracle's action

under the cfg mask with exact_ties = 0 (the set split where one fingerprint appears under two auxkeys) and exact_ties = 1, through the probe
(probe_violators = the oracle's set), and under every single-bit mask whose bit occurs.  A verdict is the oracle's with every invariant
evaluated alone; an evaluation that raises counts as a violation of that bit (the kernels' documented rule).

usage: model_seeded_worker.py MODEL(2|3) out.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# (space, base states walked for latent parents): the shipped constants (the specialised k_expand) and the three-value space (the generic one)
SEED_SPACES = (("r3v2", 2000), ("r3v3", 2000))


def main():
    model, out_path = int(sys.argv[1]), sys.argv[2]
    import vsr_tlaplus_amd as vt
    import invariant_mutants as im
    from deep_seeded_worker import Case, make_checker, parts_without_ties, run_step
    assert getattr(vt.load(), "vsrmc_test_checker_seed_records", None) is not None, "run me with VSRMC_LIB = libvsrmc_hooks.so"
    orc, _po = im.MODELS[model]
    out = dict(model=model, seeds=0, runs=[], bits_that_occur=[])
    occur = set()
    for space, take in SEED_SPACES:
        R, values, L, _depth = im.SPACES[space]
        key = (R, len(values), L)
        recs, fps = [], set()
        for m in im.latent_parents(model, space, take):              # aux_client_acked is no part of the VIEW: one seed per fingerprint
            fp = orc.fingerprint(im.oracle_params(model, space, 0), m.words)[0]
            if fp not in fps:
                fps.add(fp)
                recs.append(m.words)
        succ = [orc.successors(im.oracle_params(model, space, 0), r) for r in recs]
        memo = {}

        def verdict(words, mask, space=space, memo=memo):
            k = tuple(int(x) for x in words)
            if k not in memo:
                memo[k] = im.orc_verdicts(model, space, words)
            return sum(b for b, v in memo[k].items() if (mask & b) and v != 0)

        def make_model(vt, mask, key=key):
            return (vt.Model.second_model if model == 2 else vt.Model.third_model)(R=key[0], n=key[1], L=key[2], invariant_mask=mask)
        kw = dict(make_model=make_model, verdict=verdict)
        cfg = im.CFG_MASK[model]
        parts, left = parts_without_ties(orc, key, recs, succ, **kw)
        assert left * 100 <= len(recs), ("more than 1 % of the seeds left out of the single-pass run", left, len(recs))
        print("%s: seeds %d, parts %s, left out of the single-pass run %d" % (space, len(recs), [len(p) for p in parts], left), flush=True)
        out["seeds"] += len(recs)
        whole = Case(orc, key, recs, succ, im.ALL_MASK[model], **kw)
        bits = [b for b in im.BITS[model] if any(v & b for v in whole.viol.values())]
        occur.update(bits)
        assert whole.viol, "no violating successor: the checks would be vacuous"
        for mask in [cfg] + bits:
            for k, part in enumerate(parts):
                r = run_step(vt, orc, key, [recs[i] for i in part], [succ[i] for i in part], 0, inv_mask=mask,
                             label="%s mask %d exact_ties=0 part %d" % (space, mask, k), **kw)
                out["runs"].append(dict(r, mask=mask, space=space))
                print(json.dumps(out["runs"][-1]), flush=True)
        r = run_step(vt, orc, key, recs, succ, 1, inv_mask=cfg, label="%s mask %d exact_ties=1" % (space, cfg), **kw)
        out["runs"].append(dict(r, mask=cfg, space=space))
        print(json.dumps(out["runs"][-1]), flush=True)
        # the probe over the seeded level: counts, the smallest violator, the whole violator list
        for mask in [cfg] + bits:
            case = Case(orc, key, recs, succ, mask, **kw)
            m, mc = make_checker(vt, case, 0)
            try:
                mc.seed_records(*case.batch())
                p = mc.probe()
                vmask = 0
                for v in case.viol.values():
                    vmask |= v
                assert case.viol or mask == cfg
                want = (case.generated, min(case.viol), vmask) if case.viol else (case.generated, (1 << 64) - 1, 0)
                assert (p["generated"], p["viol_fp"], p["viol_mask"]) == want, (space, mask, p, want)
                assert mc.probe_violators() == sorted(case.viol), (space, mask)
                print("%s mask %d probe: generated %d, violators %d" % (space, mask, p["generated"], len(case.viol)), flush=True)
            finally:
                mc.close()
                m.close()
    out["bits_that_occur"] = sorted(occur)
    with open(out_path, "w") as f:
        json.dump(out, f)
    print("ok", flush=True)


if __name__ == "__main__":
    main()
