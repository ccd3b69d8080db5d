#!/usr/bin/env python3
"""tools/bench_action_constraint.py [OUT.json] [MAX_SECONDS] — what an action constraint costs per level on BASELINE config 2.

Three runs in one process under the automatic level scheme (buffers sized from the free HBM), one after the other:
  plain                  no constraint: `expand_ms` of the k_expand launch(es) of every level — the yardstick
  TRUE                   the constraint that blocks nothing: every level goes through k_step_list / k_step_apply / k_step_expand instead
  CommitNeverDecreases   replicas never lower their commit number: how much of config 2 remains, and whether the violation survives
For every level above 10^6 states of the two constrained runs one JSON line: the HIP-event ms of the three stages, slices, slices listed again, launches,
transitions generated / blocked, and beside them the plain run's expand_ms for the level of the same number with `gated_over_k_expand` = the ratio of the
three stages' sum to it (for CommitNeverDecreases the levels are not the same sets: the ratio is there for orientation only).  Then one closing line per
run.  Lines go to stdout and are appended to OUT.json when given (profiles/action_constraint_cost.json holds such lines).  A run ends at a violation, when
the search is exhausted, when the next level does not fit, or after MAX_SECONDS (default 150)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_tlaplus_amd as vt  # noqa: E402

RUNS = [
    ("plain", None),
    ("TRUE", r"Everything == TRUE"),
    ("CommitNeverDecreases", r"CommitNeverDecreases == \A r \in replicas : rep_commit_number'[r] >= rep_commit_number[r]"),
]


def main():
    out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    max_seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 150.0

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    model = vt.Model.from_constants(R=3, C_=1, n=2, L=2)
    plain = {}                                                     # level -> (states expanded, generated, expand_ms) of the unconstrained run
    for name, text in RUNS:
        mc = vt.ModelChecker.auto(model, device=0)
        if text is not None:
            mc.action_constrain(model.compile_step_predicates(text))
        t0 = time.time()
        end = "max-seconds"
        while time.time() - t0 < max_seconds:
            if mc.room() == 2:
                end = "seen-set-full"
                break
            parents = mc.n_frontier
            kind, d, _p = mc.advance()
            if kind == "stopped":
                end = "out-of-room: " + mc.stopped
                break
            if kind != "level":
                end = "beyond the record buffers at level %d" % d["level"]
                break
            if text is None:
                plain[d["level"]] = (parents, d["generated"], d["expand_ms"])
            elif parents >= 10 ** 6:
                ai = mc.action_constraint_results(0)
                gated = ai["list_ms"] + ai["verdict_ms"] + ai["expand_ms"]
                ref = plain.get(ai["level"])
                emit(dict(run=name, level=ai["level"], parents=parents, generated=ai["pairs"], blocked=ai["blocked"], new=d["n_new"], list_ms=round(ai["list_ms"], 3),
                          verdict_ms=round(ai["verdict_ms"], 3), expand_ms=round(ai["expand_ms"], 3), gated_ms=round(gated, 3), slices=ai["slices"],
                          relisted=ai["relisted"], launches=ai["launches"], level_seconds=round(d["seconds"], 4),
                          k_expand_parents=ref[0] if ref else None, k_expand_ms=round(ref[2], 3) if ref else None,
                          gated_over_k_expand=round(gated / ref[2], 2) if ref and ref[2] else None))
            if mc.violation is not None:
                end = "violation at level %d (mask %d)" % (mc.violation["level"], mc.violation["mask"])
                break
            if d["n_new"] == 0:
                end = "exhausted"
                break
        row = dict(run=name, end=end, depth=mc.depth, distinct=mc.distinct, seconds=round(time.time() - t0, 2))
        if text is not None:
            rs = mc.action_constraint_results()
            row.update(blocked=sum(r["blocked"] for r in rs), blocked_violating=sum(r["blocked_violating"] for r in rs),
                       blocked_act={a: sum(r["blocked_act"].get(a, 0) for r in rs) for a in sorted(set(a for r in rs for a in r["blocked_act"]))},
                       gated_ms=round(sum(r["list_ms"] + r["verdict_ms"] + r["expand_ms"] for r in rs), 1), slices=sum(r["slices"] for r in rs),
                       launches=sum(r["launches"] for r in rs))
        else:
            row.update(k_expand_ms=round(sum(v[2] for v in plain.values()), 1))
        emit(row)
        mc.close()


if __name__ == "__main__":
    main()
