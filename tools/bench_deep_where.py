#!/usr/bin/env python3
"""tools/bench_deep_where.py [config2|readme] [OUT.json] [LAST_LEVEL] — what a user's predicates cost on the levels beyond the record buffers.

Runs the configuration to LAST_LEVEL (config 2 with small record buffers, so that the search leaves them early: default 16; the README configuration under
the automatic level scheme: default 23, which probes level 24) four ways in one process and one build: unattached, with the state predicate LogDivergence
attached, with the step predicate CommittedPrefixStable attached, and with both.  One warm-up run, then three of each, and the median of the wall-clock time
of the deepen passes alone (the stored levels are the same work in every variant).  Per variant one JSON line on stdout, appended to OUT.json when given
(profiles/deep_where.json holds such lines): the median, the raw times, and for the attached variants the per-level counts with their `exact` flags —
the probed level's counts are lower bounds when the list of collected copies overflowed, and the line says so."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vsr_tlaplus_amd as vt  # noqa: E402

CONFIGS = dict(config2=(dict(R=3, C_=1, n=2, L=2), dict(table_log2=26, frontier_words=1 << 24, frontier_states=1 << 19, pending_entries=1 << 20), 16),
               readme=(dict(R=3, C_=1, n=3, L=3), None, 23))
LOG_DIVERGENCE = (r"LogDivergence == \E r1, r2 \in replicas : \E i \in DOMAIN rep_log[r1] : i \in DOMAIN rep_log[r2] /\ rep_log[r1][i] # rep_log[r2][i]")
COMMITTED_PREFIX_STABLE = (r"CommittedPrefixStable == \A r \in replicas : \A i \in DOMAIN rep_log[r] : i <= rep_commit_number[r] => "
                           r"(i \in DOMAIN rep_log'[r] /\ rep_log[r][i]' = rep_log[r][i])")


def one_run(model, sizes, last, state, step):
    mc = vt.ModelChecker(model, **sizes) if sizes else vt.ModelChecker.auto(model, device=0)
    if state is not None or step is not None:
        mc.deep_attach(state, step)
    deep_s, n_deep = 0.0, 0
    while mc.depth < last and mc.violation is None:
        if mc.room() == 2:
            break
        t0 = time.time()
        kind, d, _p = mc.advance()
        if kind == "deep":
            deep_s += time.time() - t0
            n_deep += 1
        if d["n_new"] == 0:
            break
    res = mc.deep_results() if (state is not None or step is not None) else []
    out = dict(deep_seconds=deep_s, deep_passes=n_deep, depth=mc.depth, stored_through=mc.level, distinct=mc.distinct,
               levels=[dict(level=r["level"], kind=r["kind"], exact=r["exact"], state=r["state"] and r["state"]["count"], step=r["step"] and r["step"]["count"],
                            pairs=r["step"] and r["step"]["n_pairs"], where_ms=r["where_ms"], step_ms=r["step_ms"]) for r in res])
    mc.close()
    return out


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "config2"
    out = open(sys.argv[2], "a") if len(sys.argv) > 2 else None
    consts, sizes, last = CONFIGS[which]
    if len(sys.argv) > 3:
        last = int(sys.argv[3])
    model = vt.Model.from_constants(**consts)
    state, step = model.compile_where(LOG_DIVERGENCE), model.compile_step(COMMITTED_PREFIX_STABLE)
    one_run(model, sizes, last, None, None)                            # warm-up
    base = None
    for name, s, p in (("unattached", None, None), ("LogDivergence", state, None), ("CommittedPrefixStable", None, step), ("both", state, step)):
        runs = [one_run(model, sizes, last, s, p) for _ in range(3)]
        times = [r["deep_seconds"] for r in runs]
        med = statistics.median(times)
        base = med if base is None else base
        row = dict(config=which, variant=name, last_level=last, deep_seconds=times, median_s=med, ratio_to_unattached=med / base if base else None, **{
            k: runs[-1][k] for k in ("deep_passes", "depth", "stored_through", "distinct", "levels")})
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
