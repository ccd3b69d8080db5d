#!/usr/bin/env python3
"""tools/bench_deep_constrain.py cost|config5|off [OUT.json] — the measurements of DESIGN.md §9l: what a state constraint costs on the levels beyond the
record buffers, and how deep BASELINE configs[4] ("config 5") gets under one.  One JSON line per row on stdout, appended to OUT.json when given
(profiles/deep_constrain.json holds such lines).  Every row is ONE run unless it says otherwise.

    cost     config 2 (small record buffers, so that the search leaves them early; to level 20) and config 5 (sized from the free HBM, as far as
             tools/run_config5.py goes) through the automatic level scheme, unconstrained and with `True` attached and the opt-in on, in one process and
             one build, the two alternating after a warm-up: wall-clock seconds of the deep passes alone, the ratio, and that every figure agrees.
    config5  config 5 under Replica3Normal with the opt-in on, until the search is exhausted, the seen-set is full or --max-seconds have passed: the depth
             reached, kept / pruned per level, and the share of the regenerated records that are pruned ones (judged again in every descent).
    off      prints the command lines of the off-means-off measurement: `bench.py --gpus 1 --steps 5 --warmup 2` on this build and on a build of the
             parent commit, alternating in one job; the margin is the spread the parent shows between its own rounds in that job."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_tlaplus_amd as vt  # noqa: E402

CONFIGS = dict(config2=(dict(R=3, C_=1, n=2, L=2), dict(table_log2=26, frontier_words=1 << 24, frontier_states=1 << 19, pending_entries=1 << 20), 20),
               config5=(dict(R=5, C_=1, n=2, L=2), None, 14))
TRUE = "True == TRUE"
R3N = "Replica3Normal == rep_status[3] = Normal"


def checker(model, sizes, text):
    mc = vt.ModelChecker(model, **sizes) if sizes else vt.ModelChecker.auto(model, device=0)
    if text is not None:
        mc.constrain(model.compile_predicates(text), deep=True)
    return mc


def run(model, sizes, last, text, max_seconds=None, stop_before_overfill=False):
    mc = checker(model, sizes, text)
    slots = 1 << int(mc.options.table_log2)
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
        # tools/run_config5.py's rule: will the next pass overfill a seen-set that cannot grow?  (the last level's growth bounds the next one's; under a
        # constraint the pruned states take slots too: the level's written size is what counts)
        deep = [x for x in passes if x["kind"] == "deep"]
        if stop_before_overfill and len(deep) >= 2 and deep[-2]["n_new"]:
            slots = 1 << int(mc.options.table_log2)
            nxt = deep[-1]["n_new"] * deep[-1]["n_new"] / deep[-2]["n_new"]
            if mc.distinct + pruned_so_far(mc, text) + nxt > 0.85 * slots:
                stop = "seen-set-full (the next level would not fit: %d slots)" % slots
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
    out = dict(stop=stop, depth=mc.depth, table_slots=slots, stored_through=mc.level, distinct=mc.distinct, deep_seconds=deep_s, seconds=time.time() - t_start, passes=passes,
               rebased=[r["level"] for r in mc.rebased])
    if text is not None:
        out["levels"] = [dict(level=r["level"], kept=r["kept"], pruned=r["pruned"]) for r in mc.constraint_results()]
        out["deep_levels"] = mc.constraint_deep_results()
    mc.close()
    return out


def pruned_so_far(mc, text):
    return sum(r["pruned"] for r in mc.constraint_results()) if text is not None else 0


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def cost(out):
    for which in ("config2", "config5"):
        consts, sizes, last = CONFIGS[which]
        model = vt.Model.from_constants(**consts)
        run(model, sizes, min(last, 12), None)                       # warm-up
        plain = run(model, sizes, last, None)
        true = run(model, sizes, last, TRUE)
        same = [(a["level"], a["n_new"], a["generated"], a["distinct"], a["fp_xor"]) for a in plain["passes"]] == \
               [(a["level"], a["n_new"], a["generated"], a["distinct"], a["fp_xor"]) for a in true["passes"]]
        emit(dict(measurement="cost of the filter (one run each)", config=which, last_level=last, figures_agree=same, pruned=sum(r["pruned"] for r in true["levels"]),
                  deep_seconds_unconstrained=plain["deep_seconds"], deep_seconds_true=true["deep_seconds"],
                  ratio=true["deep_seconds"] / plain["deep_seconds"] if plain["deep_seconds"] else None,
                  filter_launches=sum(d["launches"] for d in true["deep_levels"]), unconstrained=plain, true=true), out)


def config5(out, max_seconds):
    consts, sizes, _last = CONFIGS["config5"]
    model = vt.Model.from_constants(**consts)
    r = run(model, sizes, None, R3N, max_seconds=max_seconds, stop_before_overfill=True)
    regen = sum(d["regen_records"] for d in r["deep_levels"])
    pruned = sum(d["regen_pruned"] for d in r["deep_levels"])
    emit(dict(measurement="config 5 under Replica3Normal, opt-in on (one run)", stop=r["stop"], depth=r["depth"], stored_through=r["stored_through"], distinct=r["distinct"],
              pruned=sum(l["pruned"] for l in r["levels"]), seconds=r["seconds"], deep_seconds=r["deep_seconds"], regenerated_records=regen,
              regenerated_pruned=pruned, pruned_share_of_regenerated=pruned / regen if regen else None, rebased=r["rebased"], levels=r["levels"],
              deep_levels=r["deep_levels"], passes=r["passes"]), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["cost", "config5", "off"])
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
        config5(out, a.max_seconds)


if __name__ == "__main__":
    main()
