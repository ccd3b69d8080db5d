#!/usr/bin/env python3
"""tools/bench_terminal.py [config2|readme] [OUT.json] — what the guards-only scan for terminal states costs.

Runs the configuration under the automatic level scheme (buffers sized from the free HBM) and, on every stored level above 10^7 states, times
k_terminal (vsrmc_checker_terminal_scan: HIP-event time of the kernel; one warm-up launch, then 5, and their median) against `expand_ms` of the
k_expand launch that then expands the same level, in the same run.  Asserts on every such level that the scan's n_terminal equals that step's
`deadlocks`.  One JSON line per level on stdout, appended to OUT.json when given (profiles/terminal_scan.json holds such lines)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_tlaplus_amd as vt  # noqa: E402

CONFIGS = dict(config2=dict(R=3, C_=1, n=2, L=2), readme=dict(R=3, C_=1, n=3, L=3))


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "config2"
    out = open(sys.argv[2], "a") if len(sys.argv) > 2 else None
    mc = vt.ModelChecker.auto(vt.Model.from_constants(**CONFIGS[which]), device=0)
    while True:
        row = None
        if mc.n_frontier > 10 ** 7 and mc.depth == mc.level:
            ms = []
            for rep in range(6):
                t = mc.terminal_scan()
                if rep:
                    ms.append(t["kernel_ms"])
            row = dict(config=which, level=mc.level, states=mc.n_frontier, scan_ms=ms, scan_median_ms=statistics.median(ms),
                       n_terminal=t["n_terminal"], n_unsettled=t["n_unsettled"], min_fp=t["min_fp"])
        if mc.room() == 2:
            break
        kind, d, _p = mc.advance()
        if row is not None:
            row.update(expanded_by=kind, expand_ms=d["expand_ms"], deadlocks=d["deadlocks"],
                       next_level_record_words=mc.levels[-1].get("record_words") if kind == "level" else None)
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
