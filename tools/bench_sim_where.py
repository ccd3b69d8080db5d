#!/usr/bin/env python3
"""tools/bench_sim_where.py [OUT.json] [SECONDS] — what a user's predicate on every walk costs the simulation mode.

The README configuration (3,1,3,3), 2^17 walkers, depth 60, seed 2, no built-in invariant (invariant_mask = 0: nothing ends a run early), a fixed
SECONDS (default 5) per run.  The yardstick is steps/s of vsrmc_simulate (k_simulate: the parent's kernel and host loop, untouched).  Against it
vsrmc_simulate_where in report mode (stop = 0) with the three state predicates of tools/bench_where.py — replica words only, a quantifier over a log's
positions, a quantifier over DOMAIN messages — each alone, and with CommittedPrefixStable of tools/steps_example.txt as a step program.  Every figure is
the median of 5 runs after one warm-up run.  One JSON line per variant on stdout, appended to OUT.json when given (profiles/sim_where.json holds such
lines)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import vsr_tlaplus_amd as vt  # noqa: E402
from bench_where import PREDICATES  # noqa: E402

KW = dict(n_walkers=1 << 17, max_depth=60, seed=2)
COMMITTED_PREFIX_STABLE = (r"CommittedPrefixStable == \A r \in replicas : \A i \in DOMAIN rep_log[r] : i <= rep_commit_number[r] => "
                           r"(i \in DOMAIN rep_log'[r] /\ rep_log'[r][i] = rep_log[r][i])")


def main():
    out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 5.0
    m = vt.Model.from_constants(R=3, C_=1, n=3, L=3, invariant_mask=0)
    variants = [("simulate", None, lambda: m.simulate(max_seconds=seconds, **KW))]
    for name, text in PREDICATES:
        w = m.compile_predicates(text)
        variants.append(("state_" + name, w, (lambda w: lambda: m.simulate_where(state=w, stop=False, max_seconds=seconds, **KW))(w)))
    ws = m.compile_step_predicates(COMMITTED_PREFIX_STABLE)
    variants.append(("step_CommittedPrefixStable", ws, lambda: m.simulate_where(step=ws, stop=False, max_seconds=seconds, **KW)))
    base = None
    for name, w, run in variants:
        rates, last = [], None
        for rep in range(6):
            last = run()
            assert last["found"] == 0, last
            if rep:
                rates.append(last["steps"] / last["seconds"])
        row = dict(variant=name, config="readme", seconds=seconds, steps_per_s=rates, median_steps_per_s=statistics.median(rates), **KW)
        if w is not None:
            d = w.describe()
            row.update(n_ops=d["n_ops"], depth=d["depth"], msg_loops=d["msg_loops"], count=list((last["count_state"] or last["count_step"]).values())[0],
                       evaluated=last["n_states"] or last["n_pairs"])
        if base is None:
            base = row["median_steps_per_s"]
        row["bare_walk_over_this"] = base / row["median_steps_per_s"]
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
