#!/usr/bin/env python3
"""tools/bench_where_models.py [second|third] [OUT.json] — what evaluating a user's state predicates costs on the two analysis models.

Runs the model under the constants of its shipped cfg (3 replicas, two values, limit 2) and the automatic level scheme.  On EVERY stored level it scans
once with the example predicates (what -whereReport prints: the "report" lines).  On six consecutive stored levels of at least 10^7 states it times, in
the same run: k_terminal<MODEL> (vsrmc_checker_terminal_scan — the parent's kernel, untouched: the yardstick), k_where<MODEL> for a replica-word
predicate (InStateTransfer), a log predicate (LogDivergence), a message-loop predicate (DvcLogBelowCommit) and, on the third model, a held-DoViewChange
predicate (HeldDvcShorterLog), and `expand_ms` of the k_expand launch that then expands the level.  Every scan figure is the HIP-event time of the kernel:
one warm-up launch, then 5, and their median.  One JSON line per level on stdout, appended to OUT.json when given (profiles/where_models.json)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_tlaplus_amd as vt  # noqa: E402

PREDICATES = [
    ("replica", "InStateTransfer", r"\E r \in replicas : rep_status[r] = StateTransfer"),
    ("log", "LogDivergence", r"\E r1, r2 \in replicas : \E i \in DOMAIN rep_log[r1] : i \in DOMAIN rep_log[r2] /\ rep_log[r1][i] # rep_log[r2][i]"),
    ("message", "DvcLogBelowCommit", r"\E m \in DOMAIN messages : m.type = DoViewChangeMsg /\ (\E r \in replicas : rep_commit_number[r] > Len(m.log))"),
]
HELD = ("held", "HeldDvcShorterLog", r"\E r \in replicas : \E d \in rep_recv_dvc[r] : Len(d.log) < Len(rep_log[r])")
TIMED_LEVELS = 6


def median_ms(scan):
    ms = []
    for rep in range(6):
        t = scan()
        if rep:
            ms.append(t["kernel_ms"])
    return t, ms


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "second"
    out = open(sys.argv[2], "a") if len(sys.argv) > 2 else None
    model = vt.Model.second_model(R=3, n=2, L=2) if which == "second" else vt.Model.third_model(R=3, n=2, L=2)
    example = open(os.path.join(ROOT, "tools", "predicates_model%d_example.txt" % (2 if which == "second" else 3))).read()
    report = model.compile_predicates(example)
    compiled = [(tag, name, model.compile_predicates(text)) for tag, name, text in PREDICATES + ([HELD] if which == "third" else [])]

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    mc = vt.ModelChecker.auto(model, device=0)
    timed = 0
    while timed < TIMED_LEVELS:
        row = None
        if mc.depth == mc.level and mc.n_frontier:
            t = mc.where_scan(report)
            emit(dict(model=which, report=True, level=t["level"], states=t["n_states"], where=dict(zip(report.names, t["count"]))))
            if mc.n_frontier >= 10 ** 7:
                t, ms = median_ms(mc.terminal_scan)
                row = dict(model=which, level=mc.level, states=mc.n_frontier, terminal_ms=ms, terminal_median_ms=statistics.median(ms), n_terminal=t["n_terminal"])
                for tag, name, w in compiled:
                    t, ms = median_ms(lambda: mc.where_scan(w))
                    d = w.describe()
                    row["where_" + tag] = dict(name=name, ms=ms, median_ms=statistics.median(ms), hits=t["count"][0], min_fp=t["min_fp"][0], n_ops=d["n_ops"],
                                               depth=d["depth"], msg_loops=d["msg_loops"])
        elif mc.depth != mc.level:
            emit(dict(model=which, report=True, level=mc.depth, stored=False))
        if mc.room() == 2:
            break
        kind, d, _p = mc.advance()
        if row is not None:
            row.update(expanded_by=kind, expand_ms=d["expand_ms"], deadlocks=d["deadlocks"])
            if kind == "level":
                assert d["deadlocks"] == row["n_terminal"], row
            emit(row)
            timed += 1
        if kind != "level" or d["n_new"] == 0 or mc.violation is not None:
            break
    mc.close()


if __name__ == "__main__":
    main()
