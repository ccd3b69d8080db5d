#!/usr/bin/env python3
"""tools/bench_where.py [config2|readme] [OUT.json] — what evaluating a user's state predicates on a stored level costs.

Runs the configuration under the automatic level scheme (buffers sized from the free HBM) and, on every stored level above 10^7 states, times in one
run: k_terminal (vsrmc_checker_terminal_scan — the parent's kernel, untouched: the yardstick), k_where (vsrmc_checker_where_scan) for three predicates
of rising reach — replica words only, with a quantifier over a log's positions, with one quantifier over DOMAIN messages — and `expand_ms` of the
k_expand launch that then expands the same level.  Every scan figure is the HIP-event time of the kernel: one warm-up launch, then 5, and their
median.  One JSON line per level on stdout, appended to OUT.json when given (profiles/where_scan.json holds such lines)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_tlaplus_amd as vt  # noqa: E402

CONFIGS = dict(config2=dict(R=3, C_=1, n=2, L=2), readme=dict(R=3, C_=1, n=3, L=3))
PREDICATES = [
    ("replica", r"\E r1, r2 \in replicas : rep_status[r1] = Normal /\ rep_status[r2] = Normal /\ rep_view_number[r1] # rep_view_number[r2]"),
    ("log", r"\E r1, r2 \in replicas : \E i \in DOMAIN rep_log[r1] : i \in DOMAIN rep_log[r2] /\ rep_log[r1][i] # rep_log[r2][i]"),
    ("message", r"\E m \in DOMAIN messages : m.type = StartViewMsg /\ messages[m] >= 1 /\ rep_view_number[m.dest] > m.view_number"),
]


def median_ms(scan):
    ms = []
    for rep in range(6):
        t = scan()
        if rep:
            ms.append(t["kernel_ms"])
    return t, ms


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "config2"
    out = open(sys.argv[2], "a") if len(sys.argv) > 2 else None
    model = vt.Model.from_constants(**CONFIGS[which])
    compiled = [(name, model.compile_where(text)) for name, text in PREDICATES]
    mc = vt.ModelChecker.auto(model, device=0)
    while True:
        row = None
        if mc.n_frontier > 10 ** 7 and mc.depth == mc.level:
            t, ms = median_ms(mc.terminal_scan)
            row = dict(config=which, level=mc.level, states=mc.n_frontier, terminal_ms=ms, terminal_median_ms=statistics.median(ms), n_terminal=t["n_terminal"])
            for name, w in compiled:
                t, ms = median_ms(lambda: mc.where_scan(w))
                d = w.describe()
                row["where_" + name] = dict(ms=ms, median_ms=statistics.median(ms), hits=t["count"][0], min_fp=t["min_fp"][0], n_ops=d["n_ops"], depth=d["depth"],
                                            msg_loops=d["msg_loops"])
        if mc.room() == 2:
            break
        kind, d, _p = mc.advance()
        if row is not None:
            row.update(expanded_by=kind, expand_ms=d["expand_ms"], deadlocks=d["deadlocks"])
            if kind == "level":
                assert d["deadlocks"] == row["n_terminal"], row
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        if kind != "level" or d["n_new"] == 0 or mc.violation is not None:
            break
    mc.close()


if __name__ == "__main__":
    main()
