#!/usr/bin/env python3
"""tools/bench_sim_constrained.py [OUT.json] [SECONDS] — what walking under constraints costs the simulation mode.

The README configuration (3,1,3,3), 2^17 walkers, depth 60, seed 2, no built-in invariant (invariant_mask = 0: nothing ends a run early), report mode, a
fixed SECONDS (default 3) per run.  The yardstick is steps/s of vsrmc_simulate_where (k_simulate_where, untouched) with a one-predicate state program and a
one-predicate step program, both TRUE.  Against it vsrmc_simulate_constrained with the same two programs as `always` constraints: the same number of
interpreter calls per iteration, so the difference is the tried set and the undo log.  Then with constraints that bite: Replica3Normal
(tools/constraints_example.txt) as the state constraint, QuietClient (tools/action_constraints_example.txt) as the action constraint, and both — there an
iteration may be a refused try, so `tries_per_s` (steps + blocked + pruned per second) stands beside steps/s.  Every figure is the median of 5 runs after
one warm-up run.  One JSON line per variant on stdout, appended to OUT.json when given (profiles/sim_constrained.json holds such lines)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_tlaplus_amd as vt  # noqa: E402

KW = dict(n_walkers=1 << 17, max_depth=60, seed=2, stop=False)
TRUE = "Always == TRUE"
REPLICA3_NORMAL = "Replica3Normal == rep_status[3] = Normal"
QUIET_CLIENT = r"QuietClient == step_action = ReceiveClientRequest => \A m \in DOMAIN messages : messages[m] = 0"


def main():
    out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 3.0
    m = vt.Model.from_constants(R=3, C_=1, n=3, L=3, invariant_mask=0)
    s_true, p_true = m.compile_predicates(TRUE), m.compile_step_predicates(TRUE)
    s_r3n, p_quiet = m.compile_predicates(REPLICA3_NORMAL), m.compile_step_predicates(QUIET_CLIENT)
    con = lambda s, p: (lambda: m.simulate_constrained(state=s, constraint=0, step=p, action_constraint=0, max_seconds=seconds, **KW))   # noqa: E731
    variants = [("simulate_where_true_true", lambda: m.simulate_where(state=s_true, step=p_true, max_seconds=seconds, **KW)),
                ("constrained_always_always", con(s_true, p_true)),
                ("constrained_Replica3Normal_always", con(s_r3n, p_true)),
                ("constrained_always_QuietClient", con(s_true, p_quiet)),
                ("constrained_Replica3Normal_QuietClient", con(s_r3n, p_quiet))]
    base = None
    for name, run in variants:
        rates, tries, last = [], [], None
        for rep in range(6):
            last = run()
            assert last["found"] == 0, last
            if rep:
                rates.append(last["steps"] / last["seconds"])
                tries.append((last["steps"] + last.get("blocked", 0) + last.get("pruned", 0)) / last["seconds"])
        row = dict(variant=name, config="readme", seconds=seconds, steps_per_s=rates, median_steps_per_s=statistics.median(rates),
                   median_tries_per_s=statistics.median(tries), rounds=last["rounds"], steps=last["steps"], walks=last["walks"], blocked=last.get("blocked", 0),
                   pruned=last.get("pruned", 0), stuck=last.get("stuck", 0), **{k: v for k, v in KW.items() if k != "stop"})
        if base is None:
            base = row["median_steps_per_s"]
        row["baseline_steps_over_this"] = base / row["median_steps_per_s"]
        row["baseline_steps_over_these_tries"] = base / row["median_tries_per_s"]
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
