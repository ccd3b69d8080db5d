#!/usr/bin/env python3
"""tools/bench_step_models.py [second|third] [OUT.json] [TIMED_LEVELS] — what evaluating a user's step predicates costs on the two analysis models
(DESIGN.md §9e).

Runs the model under the constants of its shipped cfg (3 replicas, two values, limit 2) and the automatic level scheme.  On EVERY stored level it scans
once with the example step predicates (what -stepReport prints: the "report" lines, with the action of each property's witness).  On TIMED_LEVELS
(default 6) consecutive stored levels of at least 10^7 states it times, in the same run: k_where<MODEL> for an unprimed predicate
(vsrmc_checker_where_scan), the step scan (vsrmc_checker_step_scan: k_step_list<MODEL> and k_step_apply<MODEL>, reported separately, summed over the
slices) for a replica-word predicate (commit), a log predicate (log), a loop over the successor's bag (message) and, on the third model, a predicate over
the held DoViewChanges of both sides (held), and `expand_ms` of the k_expand launch that then expands the level: the untouched yardstick.  Every scan
figure is the HIP-event time of the kernels: one warm-up scan, then 5, and their median.  One JSON line per level on stdout, appended to OUT.json when
given (profiles/step_models.json holds such lines)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_tlaplus_amd as vt  # noqa: E402

WHERE = r"\E r \in replicas : rep_status[r] = StateTransfer"
STEPS = [
    ("commit", r"\A r \in replicas : rep_commit_number'[r] >= rep_commit_number[r]"),
    ("log", r"\A r \in replicas : \A i \in DOMAIN rep_log[r] : i <= rep_commit_number[r] => (i \in DOMAIN rep_log'[r] /\ rep_log[r][i]' = rep_log[r][i])"),
    ("message", r"\E m \in DOMAIN messages' : m.type = DoViewChangeMsg /\ messages'[m] >= 1 /\ (\E r \in replicas : rep_commit_number[r] > Len(m.log))"),
]
HELD = ("held", r"\E r \in replicas : Cardinality(rep_recv_dvc[r])' < Cardinality(rep_recv_dvc[r]) \/ (\E d \in rep_recv_dvc'[r] : Len(d.log) < Len(rep_log'[r]))")


def repeat(scan, keys):
    out = {k: [] for k in keys}
    for rep in range(6):
        t = scan()
        if rep:
            for k in keys:
                out[k].append(t[k])
    return t, out


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "second"
    out = open(sys.argv[2], "a") if len(sys.argv) > 2 else None
    timed_levels = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    model = vt.Model.second_model(R=3, n=2, L=2) if which == "second" else vt.Model.third_model(R=3, n=2, L=2)
    report = model.compile_step_predicates(open(os.path.join(ROOT, "tools", "steps_model%d_example.txt" % (2 if which == "second" else 3))).read())
    where = model.compile_predicates(WHERE)
    compiled = [(name, model.compile_step_predicates(text)) for name, text in STEPS + ([HELD] if which == "third" else [])]

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    mc = vt.ModelChecker.auto(model, device=0)
    timed = 0
    while timed < timed_levels:
        row = None
        if mc.depth == mc.level and mc.n_frontier:
            t = mc.step_scan(report)
            emit(dict(model=which, report=True, level=t["level"], states=t["n_states"], pairs=t["n_pairs"], errors=t["n_err"], scan_ms=t["kernel_ms"],
                      steps=dict(zip(report.names, t["count"])),
                      witness_action=dict((n, vt.ACTION_NAMES[a]) for n, a in zip(report.names, t["min_action"]) if a is not None)))
            if mc.n_frontier >= 10 ** 7:
                t, ms = repeat(lambda: mc.where_scan(where), ["kernel_ms"])
                row = dict(model=which, level=mc.level, states=mc.n_frontier, where_ms=ms["kernel_ms"], where_median_ms=statistics.median(ms["kernel_ms"]))
                for name, w in compiled:
                    t, ms = repeat(lambda: mc.step_scan(w), ["kernel_ms", "list_ms", "apply_ms"])
                    d = w.describe()
                    row["step_" + name] = dict(ms=ms["kernel_ms"], median_ms=statistics.median(ms["kernel_ms"]), list_median_ms=statistics.median(ms["list_ms"]),
                                               apply_median_ms=statistics.median(ms["apply_ms"]), list_ms=ms["list_ms"], apply_ms=ms["apply_ms"], pairs=t["n_pairs"],
                                               errors=t["n_err"], hits=t["count"][0], min_fp=t["min_fp"][0], min_action=t["min_action"][0], slices=t["slices"],
                                               n_ops=d["n_ops"], depth=d["depth"], msg_loops=d["msg_loops"])
        elif mc.depth != mc.level:
            emit(dict(model=which, report=True, level=mc.depth, stored=False))
        if mc.room() == 2:
            break
        kind, d, _p = mc.advance()
        if row is not None:
            row.update(expanded_by=kind, expand_ms=d["expand_ms"], generated=d["generated"])
            if kind == "level":
                assert all(row["step_" + name]["pairs"] + row["step_" + name]["errors"] == d["generated"] for name, _ in compiled), row
            emit(row)
            timed += 1
        if kind != "level" or d["n_new"] == 0 or mc.violation is not None:
            break
    mc.close()


if __name__ == "__main__":
    main()
