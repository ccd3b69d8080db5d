#!/usr/bin/env python3
"""tools/bench_constrain.py [OUT.json] [MAX_SECONDS] — what a state constraint costs per level on BASELINE config 2.

Two runs under the automatic level scheme (buffers sized from the free HBM): with a constraint that prunes nothing (TRUE over a message quantifier, so that the
program is not trivial) and with Replica3Normal.  For every stored level above 10^6 states, in the same run: the HIP-event time of the ONE k_constrain launch that
filtered it (the kernel rewrites the level: it cannot be repeated), the median of five k_where launches of the same program over the same — now filtered — level
(one warm-up first), and `expand_ms` of the k_expand launch that wrote the level.  One JSON line per level on stdout, appended to OUT.json when given
(profiles/constrain_cost.json holds such lines).  A run ends when the search is exhausted, the next level does not fit, or MAX_SECONDS (default 150) have passed."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_tlaplus_amd as vt  # noqa: E402

RUNS = [
    ("prunes-nothing", r"Everything == \A m \in DOMAIN messages : m.view_number >= 0"),
    ("Replica3Normal", r"Replica3Normal == rep_status[3] = Normal"),
]


def main():
    out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    max_seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 150.0
    model = vt.Model.from_constants(R=3, C_=1, n=2, L=2)
    for name, text in RUNS:
        w = model.compile_predicates(text)
        mc = vt.ModelChecker.auto(model, device=0)
        mc.constrain(w)
        t0 = time.time()
        end = "max-seconds"
        while time.time() - t0 < max_seconds:
            if mc.room() == 2:
                end = "seen-set-full"
                break
            kind, d, _p = mc.advance()
            if kind == "stopped":
                end = "out-of-room: " + mc.stopped
                break
            if d["n_new"] == 0:
                end = "exhausted"
                break
            ci = mc.constraint_results(d["level"])
            if ci["n_states"] < 10 ** 6:
                continue
            ms = []
            for rep in range(6):
                t = mc.where_scan(w)
                if rep:
                    ms.append(t["kernel_ms"])
            assert t["n_states"] == ci["kept"] and t["count"][0] == ci["kept"], (t, ci)
            row = dict(run=name, level=d["level"], states=ci["n_states"], kept=ci["kept"], pruned=ci["pruned"], constrain_ms=ci["kernel_ms"], where_ms=ms,
                       where_median_ms=statistics.median(ms), expand_ms=d["expand_ms"], n_ops=w.describe()["n_ops"])
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        line = json.dumps(dict(run=name, end=end, depth=mc.depth, distinct=mc.distinct, pruned=sum(r["pruned"] for r in mc.constraint_results()),
                               seconds=round(time.time() - t0, 2)))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
        mc.close()


if __name__ == "__main__":
    main()
