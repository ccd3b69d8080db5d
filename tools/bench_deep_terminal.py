#!/usr/bin/env python3
"""tools/bench_deep_terminal.py [config2|readme] [OUT.json] [LAST_LEVEL] — what the deadlock check costs on the levels beyond the record buffers.

Runs the configuration to LAST_LEVEL (config 2 with small record buffers, so that the search leaves them early: default 16; the README configuration under
the automatic level scheme: default 23, which probes level 24) unattached and with the terminal attachment, in one process and one build: one warm-up run,
then three of each, and the median of the wall-clock time of the deepen passes alone.  One JSON line per variant on stdout, appended to OUT.json when given
(profiles/deep_terminal.json holds such lines).  The attached line says whether the attachment's allocation succeeded and gives per examined level:
the scan's host ms beside materialize_ms / expand_ms of the pass that scanned it; for a probed level k_step_list + k_probe_children (children_ms) and
k_terminal (ms) separately beside the probe pass, with the copies scanned and the bytes written.  n_terminal of a scanned level must equal `deadlocks` of
the pass that expands it: the tool fails where it does not."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_tlaplus_amd as vt  # noqa: E402

CONFIGS = dict(config2=(dict(R=3, C_=1, n=2, L=2), dict(table_log2=26, frontier_words=1 << 24, frontier_states=1 << 19, pending_entries=1 << 20), 16),
               readme=(dict(R=3, C_=1, n=3, L=3), None, 23))


def one_run(model, sizes, last, attach):
    mc = vt.ModelChecker(model, **sizes) if sizes else vt.ModelChecker.auto(model, device=0)
    attached = None
    if attach:
        try:
            mc.deep_terminal_attach()
            attached = True
        except vt.VsrmcError as e:                                  # (no room on the device beside the checker: recorded, the run goes on unattached)
            attached = False
            print("attachment failed: %s" % e.message, file=sys.stderr)
    deep_s, passes = 0.0, []
    while mc.depth < last and mc.violation is None:
        if mc.room() == 2:
            break
        t0 = time.time()
        kind, d, p = mc.advance()
        if kind == "deep":
            dt = time.time() - t0
            deep_s += dt
            passes.append(dict(inserted=d["level"], seconds=dt, expand_ms=d["expand_ms"], materialize_ms=d["materialize_ms"], deadlocks=d["deadlocks"],
                               probed=p["level"] if p else None, probe_ms=p["expand_ms"] if p else None))
        if d["n_new"] == 0:
            break
    levels = []
    if attached:
        by_ins = {x["inserted"]: x for x in passes}
        for r in mc.deep_terminal_results():
            row = {k: r[k] for k in ("level", "kind", "exact", "slices", "chunks", "n_states", "n_terminal", "n_unsettled", "ms", "children_ms", "bytes_written")}
            expanding = by_ins.get(r["level"] + 1)                  # the pass that inserts level + 1 expands this level
            if r["kind"] != "probed" and expanding is not None:
                row["deadlocks_of_expanding_pass"] = expanding["deadlocks"]
                assert r["n_terminal"] == expanding["deadlocks"], (r, expanding)
            levels.append(row)
    out = dict(attached=attached, deep_seconds=deep_s, depth=mc.depth, stored_through=mc.level, distinct=mc.distinct, passes=passes, levels=levels)
    mc.close()
    return out


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "config2"
    out = open(sys.argv[2], "a") if len(sys.argv) > 2 else None
    consts, sizes, last = CONFIGS[which]
    if len(sys.argv) > 3:
        last = int(sys.argv[3])
    model = vt.Model.from_constants(**consts)
    one_run(model, sizes, last, False)                               # warm-up
    base = None
    for name, attach in (("unattached", False), ("terminal", True)):
        runs = [one_run(model, sizes, last, attach) for _ in range(3)]
        times = [r["deep_seconds"] for r in runs]
        med = statistics.median(times)
        base = med if base is None else base
        row = dict(config=which, variant=name, last_level=last, deep_seconds=times, median_s=med, ratio_to_unattached=med / base if base else None,
                   **{k: runs[-1][k] for k in ("attached", "depth", "stored_through", "distinct", "passes", "levels")})
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
