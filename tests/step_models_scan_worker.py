"""Child process of test_step_models_gpu.py: the step scan of every stored level of one small space of an analysis model under the environment it was
started with (VSRMC_STEP_SLICE is read by the library at every scan) -> one JSON line: per level the scan's result without its times.  No oracle here: the
parent process compares the lines of different environments."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import vsr_tlaplus_amd as vt
    import step_models_reference as sm
    which = sys.argv[1]
    R, n, L, depth = (int(x) for x in sys.argv[2:6])
    sizes = dict(table_log2=20, frontier_words=1 << 22, frontier_states=1 << 17, pending_entries=1 << 17)
    m = (vt.Model.second_model if which == "second" else vt.Model.third_model)(R=R, n=n, L=L)
    w = m.compile_step_predicates(sm.text_of(sm.SET_A[which]))
    mc = vt.ModelChecker(m, **sizes)
    out = []
    while True:
        t = mc.step_scan(w)
        row = {k: v for k, v in t.items() if not k.endswith("_ms") and k != "slices"}
        row["slices"] = t["slices"]
        out.append(row)
        if (depth and mc.level >= depth) or mc.step()["n_new"] == 0:
            break
    mc.close()
    print("STEP_SCAN " + json.dumps(out))


if __name__ == "__main__":
    main()
