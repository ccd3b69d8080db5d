#!/usr/bin/env python3
"""tools/bench_step.py [config2|readme] [OUT.json] — what evaluating a user's step predicates on every transition out of a stored level costs
(DESIGN.md §9c).

Runs the configuration under the automatic level scheme (buffers sized from the free HBM) and, on every stored level above 10^7 states, times in one
run: k_where (vsrmc_checker_where_scan) with an unprimed predicate, the step scan (vsrmc_checker_step_scan: k_step_list and k_step_apply, reported
separately, summed over the slices) for three predicates — replica words only, log words unfolded, one quantifier over the successor's bag — and
`expand_ms` of the k_expand launch that then expands the same level: the yardstick, both enumerate and apply every instance.  Every scan figure is the
HIP-event time of the kernels: one warm-up scan, then 5, and their median.  One JSON line per level on stdout, appended to OUT.json when given
(profiles/step_scan.json holds such lines)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_tlaplus_amd as vt  # noqa: E402

CONFIGS = dict(config2=dict(R=3, C_=1, n=2, L=2), readme=dict(R=3, C_=1, n=3, L=3))
WHERE = r"\E r1, r2 \in replicas : rep_status[r1] = Normal /\ rep_status[r2] = Normal /\ rep_view_number[r1] # rep_view_number[r2]"
STEPS = [
    ("commit", r"\A r \in replicas : rep_commit_number'[r] >= rep_commit_number[r]"),
    ("log", r"\A r \in replicas : \A i \in DOMAIN rep_log[r] : rep_log'[r][i] = rep_log[r][i]"),
    ("message", r"\E m \in DOMAIN messages' : m.type = StartViewMsg /\ messages'[m] >= 1 /\ m.view_number > rep_view_number[m.dest]"),
]


def repeat(scan, keys):
    out = {k: [] for k in keys}
    for rep in range(6):
        t = scan()
        if rep:
            for k in keys:
                out[k].append(t[k])
    return t, out


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "config2"
    out = open(sys.argv[2], "a") if len(sys.argv) > 2 else None
    model = vt.Model.from_constants(**CONFIGS[which])
    where = model.compile_where(WHERE)
    compiled = [(name, model.compile_step(text)) for name, text in STEPS]
    mc = vt.ModelChecker.auto(model, device=0)
    while True:
        row = None
        if mc.n_frontier > 10 ** 7 and mc.depth == mc.level:
            t, ms = repeat(lambda: mc.where_scan(where), ["kernel_ms"])
            row = dict(config=which, level=mc.level, states=mc.n_frontier, where_ms=ms["kernel_ms"], where_median_ms=statistics.median(ms["kernel_ms"]))
            for name, w in compiled:
                t, ms = repeat(lambda: mc.step_scan(w), ["kernel_ms", "list_ms", "apply_ms"])
                d = w.describe()
                row["step_" + name] = dict(ms=ms["kernel_ms"], median_ms=statistics.median(ms["kernel_ms"]), list_median_ms=statistics.median(ms["list_ms"]),
                                           apply_median_ms=statistics.median(ms["apply_ms"]), list_ms=ms["list_ms"], apply_ms=ms["apply_ms"], pairs=t["n_pairs"],
                                           errors=t["n_err"], hits=t["count"][0], min_fp=t["min_fp"][0], min_action=t["min_action"][0], slices=t["slices"],
                                           n_ops=d["n_ops"], depth=d["depth"], msg_loops=d["msg_loops"])
        if mc.room() == 2:
            break
        kind, d, _p = mc.advance()
        if row is not None:
            row.update(expanded_by=kind, expand_ms=d["expand_ms"], generated=d["generated"])
            if kind == "level":
                assert all(row["step_" + name]["pairs"] + row["step_" + name]["errors"] == d["generated"] for name, _ in compiled), row
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
