#!/usr/bin/env python3
"""tools/bench_deep_action_constraint.py cost|readme|off [OUT.json] — the measurements of DESIGN.md §9m: what an action constraint costs on the levels beyond
the record buffers.  One JSON line per row on stdout, appended to OUT.json when given (profiles/deep_action_constraint.json holds such lines).  Every row is
ONE run.

    cost    config 2 with small record buffers, so that the search leaves them early (the setup of tools/bench_deep_constrain.py: levels 1-14 stored, 15-20
            beyond), through the automatic level scheme: unconstrained, and with `True` attached and the opt-in on, in one process and one build, after a
            warm-up.  Wall-clock seconds of the deep passes and their ratio; the gated passes' HIP-event time split into list / verdict / expand; every
            level's n_new, generated, distinct and fp_xor must agree between the two runs.
    readme  the README configuration under CommitNeverDecreases with the opt-in on, sized from the free HBM, until exhausted, a violation, a full seen-set
            or --max-seconds.
    off     prints the command lines of the off-means-off measurement: `bench.py --gpus 1 --steps 5 --warmup 2` on this build and on a build of the parent
            commit, alternating, three rounds in one job; the margin is the spread the parent shows between its own rounds in that job."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_tlaplus_amd as vt  # noqa: E402

CONFIG2 = (dict(R=3, C_=1, n=2, L=2), dict(table_log2=26, frontier_words=1 << 24, frontier_states=1 << 19, pending_entries=1 << 20), 20)
TRUE = "True == TRUE"
COMMIT = r"CommitNeverDecreases == \A r \in replicas : rep_commit_number'[r] >= rep_commit_number[r]"


def run(model, sizes, last, text, max_seconds=None):
    mc = vt.ModelChecker(model, **sizes) if sizes else vt.ModelChecker.auto(model, device=0)
    if text is not None:
        mc.action_constrain(model.compile_step_predicates(text), deep=True)
    t_start = time.time()
    deep_s, passes, stop = 0.0, [], None
    while stop is None:
        if last is not None and mc.depth >= last:
            stop = "last-level"
            break
        if max_seconds is not None and time.time() - t_start > max_seconds:
            stop = "max-seconds"
            break
        if mc.room() == 2:
            stop = "seen-set-full"
            break
        t0 = time.time()
        kind, d, p = mc.advance()
        dt = time.time() - t0
        if kind == "deep":
            deep_s += dt
        passes.append(dict(kind=kind, level=d["level"], n_new=d["n_new"], generated=d["generated"], distinct=d["distinct"], fp_xor=d["fp_xor"], seconds=round(dt, 4),
                           expand_ms=round(d["expand_ms"], 2), materialize_ms=round(d["materialize_ms"], 2), launches=d["pending"] if kind == "deep" else 1,
                           probed=p["level"] if p else None, probe_ms=round(p["expand_ms"], 2) if p else None))
        print("%s level %d: %d new, %.2f s" % (kind, d["level"], d["n_new"], dt), file=sys.stderr, flush=True)
        if d["n_new"] == 0:
            stop = "exhausted"
        elif mc.violation is not None:
            stop = "violation"
    out = dict(stop=stop, depth=mc.depth, stored_through=mc.level, distinct=mc.distinct, deep_seconds=deep_s, seconds=time.time() - t_start, passes=passes,
               rebased=[r["level"] for r in mc.rebased], violation=mc.violation)
    if text is not None:
        out["stored_levels"] = [dict(level=r["level"], blocked=r["blocked"], pairs=r["pairs"]) for r in mc.action_constraint_results()]
        out["deep_levels"] = mc.action_constraint_deep_results()
    mc.close()
    return out


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def cost(out):
    consts, sizes, last = CONFIG2
    model = vt.Model.from_constants(**consts)
    run(model, sizes, 12, None)                                      # warm-up
    run(model, dict(sizes), 12, TRUE)
    plain = run(model, sizes, last, None)
    true = run(model, sizes, last, TRUE)
    key = lambda a: (a["kind"], a["level"], a["n_new"], a["generated"], a["distinct"], a["fp_xor"])   # noqa: E731
    same = [key(a) for a in plain["passes"]] == [key(a) for a in true["passes"]]
    deep = true["deep_levels"]
    split = {k: sum(d[k] for d in deep) for k in ("list_ms", "verdict_ms", "expand_ms")}
    emit(dict(measurement="cost of the gate beyond the record buffers (one run each)", config="config2", last_level=last, figures_agree=same,
              deep_seconds_unconstrained=plain["deep_seconds"], deep_seconds_true=true["deep_seconds"],
              ratio=true["deep_seconds"] / plain["deep_seconds"] if plain["deep_seconds"] else None, gated_kernel_ms=split,
              gated_launches=sum(d["launches"] for d in deep), gated_slices=sum(d["slices"] for d in deep), unconstrained=plain, true=true), out)


def readme(out, max_seconds):
    model = vt.Model.from_constants(R=3, C_=1, n=3, L=3)
    r = run(model, None, None, COMMIT, max_seconds=max_seconds)
    emit(dict(measurement="README configuration under CommitNeverDecreases, opt-in on (one run)", **r), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["cost", "readme", "off"])
    ap.add_argument("out", nargs="?")
    ap.add_argument("--max-seconds", type=float, default=240.0)
    a = ap.parse_args()
    if a.what == "off":
        print("for round in 1 2 3; do\n  python bench.py --gpus 1 --steps 5 --warmup 2                      # this build\n"
              "  (cd PARENT_CHECKOUT && python bench.py --gpus 1 --steps 5 --warmup 2)  # the parent commit, built\ndone")
        return
    out = open(a.out, "a") if a.out else None
    if a.what == "cost":
        cost(out)
    else:
        readme(out, a.max_seconds)


if __name__ == "__main__":
    main()
