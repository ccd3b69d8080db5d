"""Child process of test_step_gpu.py: the step scan of every stored level of one small space under the environment it was started with
(VSRMC_STEP_SLICE, VSRMC_STEP_LIST_CAP are read by the library at every scan) -> one JSON line: per level the scan's result without its times, and
the hit pairs (or the error code step_pairs() raised).  No oracle here: the parent process compares the lines of different environments."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    import vsr_tlaplus_amd as vt
    import step_reference as sr
    R, C, n, L, depth = (int(x) for x in sys.argv[1:6])
    sizes = dict(table_log2=20, frontier_words=1 << 22, frontier_states=1 << 17, pending_entries=1 << 17)
    m = vt.Model.from_constants(R=R, C_=C, n=n, L=L)
    w = m.compile_step(sr.text_of(sr.SET_A))
    mc = vt.ModelChecker(m, **sizes)
    out = []
    while True:
        t = mc.step_scan(w)
        row = {k: v for k, v in t.items() if not k.endswith("_ms") and k != "slices"}
        row["slices"] = t["slices"]
        try:
            fps, ords, bits = mc.step_pairs()
            row["pairs"] = [[int(a), int(b), int(c)] for a, b, c in zip(fps, ords, bits)]
        except vt.VsrmcError as e:
            row["pairs_error"] = [e.code, e.message]
        out.append(row)
        if (depth and mc.level >= depth) or mc.step()["n_new"] == 0:
            break
    mc.close()
    print("STEP_SCAN " + json.dumps(out))


if __name__ == "__main__":
    main()
