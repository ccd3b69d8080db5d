#!/usr/bin/env python3
"""bench.py — distinct states/s and time-to-first-violation of the GPU BFS model checker on BASELINE.json's configurations.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A plain run measures the headline alone: set-up, W warm-up runs, K timed runs, the result line.  --full adds everything else this file
measures or checks: the untimed verification run and the second-hash audit, the config2 / config4 / config5 objects and the CPU
baseline.  --dump-outputs DIR (N = 1) writes what the last timed run computed as DIR/*.npy (float64; 64-bit values split into two exact
32-bit halves): per-level figures, per-action successor counts, fingerprint checksums of the levels beyond the record buffers, the
counter-example and a summary row — the same for every run of the same arguments, so two builds can be compared output for output.

N = 1.  The headline is the configuration north_star quotes the metric on and that fits one MI355X: the reference README's state-
transfer-defect configuration (BASELINE.json configs[2]: ReplicaCount=3, ClientCount=1, Values={v1,v2,v3}, StartViewOnTimerLimit=3,
VIEW + SYMMETRY on, INVARIANT AcknowledgedWriteNotLost; /root/reference/README.md:13-18).  One "step" = one complete run of the hot
path: level-synchronous BFS from Init until the first invariant violation is found and its counter-example reconstructed —
depth 24, 1 821 858 767 distinct states, 8.9e9 successors generated; the seen-set is cleared at the start of every step, HBM
allocations are reused.  No level number and no buffer size comes from this file: the checker sizes itself from the free HBM and the
automatic level scheme (ModelChecker.advance) stores a level while the next one is predicted to fit, then goes on through the seen-set
alone.  `value` = distinct states of the K timed runs / their wall time (barrier + torch.cuda.synchronize() on both sides),
`time_to_first_violation_s` = one run.  The `config2` object beside it holds the same figures for BASELINE configs[1] (the shipped
VSR.cfg constants: 28 levels, 319 228 361 distinct states) — the headline of rounds 1-2, and the headline only with --workload config2 /
--no-config3: a README leg that cannot run is an error of the bench (non-zero exit), not a reason to print another workload's number.
Inputs are the model itself (deterministic, no data files): "synthetic" in the contract's sense.  Every run asserts every level's
figures against the CPU oracle's fixtures (tests/golden/oracle_levels_config{2,3}.json); a wrong count aborts the bench.

N > 1: the SAME workload — the README defect configuration — with the seen-set sharded by the high fingerprint bits, one rank per GPU,
successors routed to their owner with an all-to-all per level / pass (vsr_tlaplus_amd/sharded_bench.py over the C++ level loop); total
work is fixed as N grows ("strong").  The automatic level scheme decides per run what is stored: at N >= 4 every level up to the
violation, at N = 2 the last levels live in the two seen-sets only.

Extra objects on the JSON line: `roofline` for the dominant kernel (k_expand: algorithmic bytes / HIP-event time on the checker's
stream; `traffic` = the committed PMC figure when it was measured on THIS build's kernel sources, else null), `cpu_baseline` = the
CPU oracle (a port, not TLC) timed on this box's host cores on a bounded sample of the headline's configuration,
`fingerprint_collision_estimate` (the birthday bound n^2 / 2^65 and TLC's d (g - d) / 2^64) and `collision_audit` (the untimed verification runs repeated under a second member
of the fingerprint family, vsrmc_model_set_fp_seed: every per-level count must equal the oracle fixture's under both).  `cpu_baseline`,
`collision_audit`, `reference_trace_in_this_run` and the config objects are --full figures.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CONFIG = dict(R=3, C=1, n=2, L=2)                     # BASELINE.json configs[1] = /root/reference/.../VSR.cfg:4-8
FP_VERSION = 2                                        # fingerprint function of this build (oracle/vsr_oracle.hpp FP_VERSION)


def load_expect():
    """What a run must reproduce, from the CPU ORACLE's run of the whole workload (tools/make_oracle_levels.py ->
    tests/golden/oracle_levels_config2*.json): level sizes, generated / deadlock counts and largest bags of all 28 levels (valid for
    any fingerprint function), and — from a fixture made with this build's fingerprint function — the per-level xor / sum of the
    fingerprints and the violating fingerprint."""
    g = os.path.join(ROOT, "tests", "golden")
    for name in ("oracle_levels_config2.json", "oracle_levels_config2_fpv1.json"):
        if os.path.exists(os.path.join(g, name)):
            with open(os.path.join(g, name)) as f:
                d = json.load(f)
            same_fp = d.get("fp_version", 1) == FP_VERSION
            return dict(distinct=d["distinct"], depth=d["depth"], levels=d["levels"], fixture=name,
                        viol_fp=int(d["viol_fp"], 16) if same_fp else None, checksums=same_fp)
    raise SystemExit("no oracle fixture for the bench workload under tests/golden/")


EXPECT = load_expect()
HBM_PEAK_GBS = 8000.0                                 # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
TABLE_LOG2 = int(os.environ.get("VSR_BENCH_TABLE_LOG2", 31))   # seen-set: 2^31 slots x 16 B = 32 GiB of the 288 GB (load 0.15 at the end)


def usable_cpus():
    """Hardware threads this process may actually use: the affinity mask, capped by the container's CPU quota (cgroup v2
    cpu.max / v1 cfs quota).  The GPU box shows 256 logical CPUs but grants 16 CPUs' worth of time: 256 oracle threads then
    run SLOWER than 16 (measured: 1.0e6 vs 2.4e6 states/s)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // p))
        except (OSError, ValueError):
            pass
    return min(n, 256)


def cpu_baseline(seconds=15.0, cfg=None):
    """CPU oracle (oracle/vsr_oracle_mt: the restatement of VSR.tla spread over std::thread workers sharing one lock-free
    seen-set, the way TLC spreads Worker threads over an FPSet) on the same config, on every CPU the container may use, for a
    bounded time."""
    exe = os.path.join(ROOT, "oracle", "build", "vsr_oracle_mt")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "-s"], check=True)
    threads = usable_cpus()
    cfg = cfg or CONFIG
    out = subprocess.run([exe, str(cfg["R"]), str(cfg["C"]), str(cfg["n"]), str(cfg["L"]), "--threads", str(threads),
                          "--max-seconds", str(seconds), "--quiet"], capture_output=True, text=True, check=True).stdout
    s = json.loads(out.strip().splitlines()[-1])
    return dict(value=round(s["states_per_s"], 1), unit="distinct states/s", cores=int(s["threads"]), kind="port",
                sample="oracle/vsr_oracle_mt (multi-threaded C++ restatement of VSR.tla, not TLC) on the headline's configuration "
                       "(R=%d, C=%d, %d values, limit %d) for %.0f s: %d distinct states, %d BFS levels"
                       % (cfg["R"], cfg["C"], cfg["n"], cfg["L"], s["seconds"], s["distinct"], s["depth"]))


AUDIT_SEED = 0x5EED5EED5EED5EED                       # second-hash audit: every count of the verification run once more under this fp_seed


def _split64(x):
    """uint64 values -> float64 [..., 2] (high, low 32-bit halves): exact, where one float64 would round them."""
    import numpy as np
    a = np.asarray(x, dtype=np.uint64)
    return np.stack([(a >> np.uint64(32)).astype(np.float64), (a & np.uint64(0xFFFFFFFF)).astype(np.float64)], axis=-1)


def run_outputs(rows, tr, distinct, depth, viol_fp):
    """What a caller of the timed path receives from one run, as float64 arrays (--dump-outputs).  rows: one (level dict, kind) per
    unit of progress, kind "level" (stored), "deep" (seen-set only: its fingerprint checksums) or "probe" (the probed level: successors
    only); tr: the counter-example [(action name, wire record)]."""
    import numpy as np
    from vsr_tlaplus_amd.checker import ACTION_NAMES
    cols = ("level", "n_new", "generated", "deadlocks", "max_bag", "viol_mask")
    levels = np.array([[float(d[c]) if kind != "probe" or c in ("level", "generated", "viol_mask") else 0.0 for c in cols]
                       for d, kind in rows], dtype=np.float64)
    acts = np.array([[float(x) for x in d["act_generated"][1:16]] for d, _kind in rows], dtype=np.float64)
    sums = np.array([[d["fp_xor"], d["fp_sum"]] if kind == "deep" else [0, 0] for d, kind in rows], dtype=np.uint64)
    recs = [np.asarray(rec, dtype=np.uint64) for _a, rec in tr]
    return {"levels": levels,                                             # columns: level, new states, generated, deadlocks, largest bag, violation mask
            "act_generated": acts,                                        # successors per action (ACTION_NAMES[1:16]) of every row of `levels`
            "fp_checksums": _split64(sums).reshape(len(rows), 4),         # xor hi, lo, sum hi, lo (0 for stored and probed levels)
            "trace_actions": np.array([ACTION_NAMES.index(a) for a, _r in tr], dtype=np.float64),
            "trace_offsets": np.cumsum([0] + [len(r) for r in recs]).astype(np.float64),
            "trace_words": _split64(np.concatenate(recs)),
            "summary": np.concatenate([np.array([distinct, depth, len(tr)], dtype=np.float64), _split64(viol_fp)])}


def dump_outputs(outputs, path):
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, a in outputs.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def run_single(args, seed=0):
    """BASELINE configs[1] through the automatic level scheme (ModelChecker.advance: every level fits the record buffers here).
    seed != 0: one untimed run under another member of the fingerprint family — every count must equal the fixture's (the
    fingerprints and checksums differ): a false merge of two states under the default function would have to repeat under this one."""
    import torch
    import vsr_tlaplus_amd as vt
    torch.cuda.set_device(0)
    m = vt.Model.from_constants(R=CONFIG["R"], C_=CONFIG["C"], n=CONFIG["n"], L=CONFIG["L"])
    if seed:
        m.set_fp_seed(seed)
    mc = vt.ModelChecker.auto(m, device=0, table_log2=TABLE_LOG2)
    S = dict(expand_ms=0.0, mat_ms=0.0, launches=0, alg_bytes=0.0, distinct=0, generated=0, ttfv=[], words=0)

    def one_run(record, verify=False):
        mc.reset()
        t0 = time.perf_counter()
        cur_words = int(m.layout.fixed_words) + int(m.layout.permutations)      # Init record, device layout
        rows = []
        while True:
            kind, d, _ = mc.advance()
            assert kind == "level", "config 2 fits the record buffers of one MI355X"
            rows.append((d, kind))
            want = EXPECT["levels"][d["level"] - 1] if d["n_new"] else None     # every run, every level: the oracle's figures
            assert want is None or (d["n_new"], d["generated"], d["deadlocks"], d["max_bag"]) == \
                (want["new"], want["generated"], want["deadlocks"], want["max_bag"]), (d["level"], d["n_new"], d["generated"])
            if verify and want is not None:                                    # untimed run: per-action counts, fingerprint checksums
                assert [int(x) for x in d["act_generated"][1:16]] == want["act_generated"][1:16], d["level"]
                x, sm, cnt = mc.level_checksum()
                assert cnt == want["new"]
                if EXPECT["checksums"] and not seed:
                    assert ("%016x" % x, "%016x" % sm) == (want["fp_xor"], want["fp_sum"]), d["level"]
            if record and d["frontier"]:
                S["expand_ms"] += d["expand_ms"]
                S["mat_ms"] += d["materialize_ms"]
                S["launches"] += 1
                # algorithmic bytes of one k_expand launch: every frontier record read once, one 8-byte
                # key read per generated successor, one 8-byte key write per newly inserted fingerprint, every new record
                # written once (single-pass levels: k_expand also materialises the successors)
                S["alg_bytes"] += 8.0 * cur_words + 8.0 * d["generated"] + 8.0 * d["n_new"] + 8.0 * d["record_words"]
                S["generated"] += d["generated"]
                S["words"] += d["record_words"]
            cur_words = d["record_words"]
            if d["n_new"] == 0 or mc.violation is not None:
                break
        if mc.violation is not None:
            tr = mc.violation_trace()                                          # counter-example reconstructed = found
            assert len(tr) == mc.violation["level"]
        dt = time.perf_counter() - t0
        assert mc.distinct == EXPECT["distinct"] and mc.level == EXPECT["depth"], (mc.distinct, mc.level)
        assert mc.violation and (seed or EXPECT["viol_fp"] is None or mc.violation["fp"] == EXPECT["viol_fp"])
        if record:
            S["distinct"] += mc.distinct
            S["ttfv"].append(dt)
            S["last"] = (rows, tr, mc.distinct, mc.level, mc.violation["fp"])    # what this run computed (--dump-outputs)

    try:
        if seed:
            one_run(False, verify=True)
            return 0.0, S, m
        if not args.no_verify:
            one_run(False, verify=True)                                        # untimed: the whole workload against the oracle fixture
        for _ in range(args.warmup):
            one_run(False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            one_run(True)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
    finally:
        mc.close()                                                             # the HBM goes to the next leg
    return elapsed, S, m


def kernel_source_sha256():
    """sha256 over the kernel sources this build was made from (csrc/*.hpp, *.hip, include/vsrmc.h, sorted by name): the committed
    PMC traffic figure (profiles/*_traffic.json) carries the hash of the sources it was measured on; another hash = another kernel =
    no traffic figure (`roofline.traffic: null`) rather than a stale one."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "vsr_tlaplus_amd", "csrc")
    for name in sorted(os.listdir(d)) + ["../../include/vsrmc.h"]:
        if name.endswith((".hpp", ".hip", ".h")):
            with open(os.path.join(d, name), "rb") as f:
                h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()


def committed_traffic(workload):
    """HBM bytes per launch of k_expand from the newest committed PMC passes for this workload ("config2" / "readme"), or None when
    they were measured on other kernel sources.  FETCH_SIZE / WRITE_SIZE cannot be read live (tools/profile_round.sh makes them)."""
    pdir = os.path.join(ROOT, "profiles")
    cands = sorted(n for n in os.listdir(pdir) if n.endswith("_traffic.json") and ("_%s_" % workload in n or (workload == "config2" and n.count("_") == 1)))
    for name in reversed(cands):
        with open(os.path.join(pdir, name)) as f:
            t = json.load(f)
        if t.get("kernel_source_sha256") == kernel_source_sha256():
            return dict(bytes_per_launch=t["hbm_bytes_per_launch"], source="PMC, profiles/%s: %s" % (name, t["source"].split(" (")[0]))
        return dict(bytes_per_launch=None, source="profiles/%s was measured on other kernel sources (sha256 %s...): no traffic figure for this build"
                                                  % (name, str(t.get("kernel_source_sha256"))[:12]))
    return dict(bytes_per_launch=None, source="no PMC passes committed for this workload")


README = dict(R=3, C=1, n=3, L=3)                     # /root/reference/README.md:13-18 = BASELINE.json configs[2]


def load_readme_expect():
    """Level figures of the README configuration: the CPU ORACLE's (tests/golden/oracle_levels_config3.json — levels 1-21 from
    oracle/vsr_oracle_mt, deeper ones from the memory-lean driver oracle/vsr_oracle_lean when the fixture holds them) and, for
    levels the oracle fixture does not reach, the GPU-sourced figures of tests/golden/config3_violation.json (marked as such)."""
    with open(os.path.join(ROOT, "tests", "golden", "oracle_levels_config3.json")) as f:
        g = json.load(f)
    with open(os.path.join(ROOT, "tests", "golden", "config3_violation.json")) as f:
        fx = json.load(f)
    levels = []
    for i, lv in enumerate(fx["levels"]):
        if i < len(g["levels"]):
            o = g["levels"][i]
            levels.append(dict(level=o["level"], n_new=o["new"], generated=o["generated"], deadlocks=o["deadlocks"], max_bag=o["max_bag"],
                               fp_xor=o.get("fp_xor"), fp_sum=o.get("fp_sum"), act_generated=o.get("act_generated"), source="oracle"))
        else:
            levels.append(dict(level=lv["level"], n_new=lv["n_new"], generated=lv["generated"], deadlocks=lv.get("deadlocks"), max_bag=lv.get("max_bag"),
                               fp_xor=None, fp_sum=None, act_generated=None, source="gpu"))
    probe = g.get("probe")                                  # the oracle's probe of level 24 (lean driver), else the GPU fixture's
    same_fp = g.get("fp_version", 1) == FP_VERSION
    return dict(levels=levels, oracle_levels=len(g["levels"]), fx=fx,
                probe_generated=(probe or fx["probe"])["generated"], probe_source="oracle" if probe else "gpu",
                viol_fp=int((probe or fx)["viol_fp"], 16) if (same_fp and fx.get("fp_version") == FP_VERSION) else None,
                checksums=same_fp)


def run_readme(args, dump_trace=None, seed=0):
    """BASELINE configs[2] = the reference README's defect configuration (3 replicas, {v1,v2,v3}, limit 3; README:13-18) on ONE GPU,
    BFS to its first violation at depth 24 through the AUTOMATIC level scheme: no level number and no buffer size comes from here.
    The checker sizes its seen-set and record buffers from the free HBM (ModelChecker.auto) and ModelChecker.advance stores a level
    while the next one is predicted to fit (levels 2-21; level 21: 261 M states, 91 GB of records), then goes on through the seen-set
    alone (csrc/vsr_deep.hpp): level 22 a virtual level, level 23 streamed through a scratch buffer from regenerated slices of level 22,
    level 24 probed — and would roll on from there had the probe come back clean.  The counter-example is reconstructed inside the
    timed region.  One step = one such run (seen-set cleared, allocations reused).  Every level figure is asserted on every run: new
    states, generated successors, deadlocks, largest bag — and, on the untimed verification run, the per-action counts and the xor /
    sum of the level's fingerprints, against the CPU oracle's fixture.  seed != 0: the verification run alone, under another member
    of the fingerprint family (counts must not change; fingerprints, checksums and the counter-example's tie-breaks do)."""
    import numpy as np
    import torch
    import vsr_tlaplus_amd as vt
    torch.cuda.set_device(0)
    E = load_readme_expect()
    deep = E["levels"]
    m = vt.Model.from_constants(R=README["R"], C_=README["C"], n=README["n"], L=README["L"])
    if seed:
        m.set_fp_seed(seed)
    t0 = time.perf_counter()
    mc = vt.ModelChecker.auto(m, device=0)
    setup = time.perf_counter() - t0
    S = dict(mat_ms=0.0, deep_ms=0.0, launches=0, alg_bytes=0.0, distinct=0, generated=0, ttfv=[], mat_s=0.0, n_mat=0, mat_levels=0,
             deep=[], same_trace=None,
             sizes=dict(table_log2=int(mc.options.table_log2), frontier_words=int(mc.options.frontier_words), frontier_states=int(mc.options.frontier_states)))

    def check_level(d, verify):
        want = deep[d["level"] - 1]
        assert (d["n_new"], d["generated"]) == (want["n_new"], want["generated"]), (d["level"], d["n_new"], d["generated"])
        if want["deadlocks"] is not None:
            assert d["deadlocks"] == want["deadlocks"], d["level"]
        if want["max_bag"] is not None:
            assert d["max_bag"] == want["max_bag"], d["level"]
        assert d["viol_mask"] == 0, d["level"]
        if verify and want["act_generated"] is not None:
            assert [int(x) for x in d["act_generated"][1:16]] == want["act_generated"][1:16], d["level"]
        return want

    def one_run(record, verify=False):
        mc.reset()
        t0 = time.perf_counter()
        cur_words = int(m.layout.fixed_words) + int(m.layout.permutations)
        alg, gen, kms, dms, launches, t_mat, n_mat, mat_levels = 0.0, 0, 0.0, 0.0, 0, 0.0, 0, 0
        # the same kernel time and algorithmic bytes once more, per KIND of pass (= per instantiation of k_expand): [ms, bytes, launches]
        split = {k_: [0.0, 0.0, 0] for k_ in ("stored", "virtual", "regenerate", "insert_beyond", "probe")}
        s_rec, n_prev = 8.0 * cur_words, 1                                   # bytes per record / states of the newest level
        passes = []
        rows = []                                                            # what the run computed, level by level (--dump-outputs)
        found = None
        while found is None:
            kind, a, b = mc.advance()
            want = check_level(a, verify)
            gen += a["generated"]
            rows.append((a, kind))
            if b is not None:
                rows.append((b, "probe"))
            if kind == "level":
                if verify and want["fp_xor"] is not None and E["checksums"] and not seed:
                    x, sm, cnt = mc.level_checksum()
                    assert cnt == want["n_new"] and ("%016x" % x, "%016x" % sm) == (want["fp_xor"], want["fp_sum"]), a["level"]
                kms += a["expand_ms"]
                launches += 1
                alg += 8.0 * cur_words + 8.0 * a["generated"] + 8.0 * a["n_new"] + 8.0 * a["record_words"]
                split["stored"][0] += a["expand_ms"]
                split["stored"][1] += 8.0 * cur_words + 8.0 * a["generated"] + 8.0 * a["n_new"] + 8.0 * a["record_words"]
                split["stored"][2] += 1
                cur_words = a["record_words"]
                s_rec, n_prev = 8.0 * a["record_words"] / a["n_new"], a["n_new"]
                n_base = a["n_new"]
                t_mat, n_mat, mat_levels = time.perf_counter() - t0, mc.distinct, a["level"]
                continue
            # a level that exists in the seen-set only.  Algorithmic bytes: SURVEY §8(d)'s B_alg = 2 S + 8 g + 8 per distinct state — every state
            # read once and written once whatever the level scheme re-expands; S = the last stored level's average record (bags grow by less
            # than one entry per level: an under-estimate of < 3 %)
            if verify and want["fp_xor"] is not None and E["checksums"] and not seed:
                assert ("%016x" % a["fp_xor"], "%016x" % a["fp_sum"]) == (want["fp_xor"], want["fp_sum"]), a["level"]
            alg += s_rec * n_prev + 8.0 * a["generated"] + 8.0 * a["n_new"] + s_rec * a["n_new"]
            # per pass: a virtual level (first pass beyond the buffers) reads its parents and claims, writes no record; a later pass regenerates the levels
            # between the base and its parents (their records written once more: the redundant work of this scheme), then inserts through a scratch buffer
            first = a["materialize_ms"] == 0.0 and b is None
            key_ = "virtual" if first else "insert_beyond"
            split[key_][0] += a["expand_ms"]
            split[key_][1] += s_rec * n_prev + 8.0 * a["generated"] + 8.0 * a["n_new"] + (0.0 if first else s_rec * a["n_new"])
            split[key_][2] += 1 if first else (a["words_new"] & 0xFFFFFFFF)
            if a["materialize_ms"]:
                split["regenerate"][0] += a["materialize_ms"]
                split["regenerate"][1] += s_rec * n_base + s_rec * n_prev      # the base level read, the level below the inserted one written (a two-level descent)
                split["regenerate"][2] += a["words_new"] >> 32
            n_prev = a["n_new"]
            dms += a["expand_ms"] + a["materialize_ms"]
            launches += a["pending"]
            row = dict(level=a["level"], seconds=a["seconds"], k_expand_ms=a["expand_ms"], regenerate_ms=a["materialize_ms"], launches=a["pending"],
                       slices=a["words_new"] >> 32, sub_slices=a["words_new"] & 0xFFFFFFFF)
            if b is not None:
                gen += b["generated"]
                alg += s_rec * n_prev + 8.0 * b["generated"]                 # the level below read, its successors looked up
                dms += b["expand_ms"]
                split["probe"][0] += b["expand_ms"]
                split["probe"][1] += s_rec * n_prev + 8.0 * b["generated"]
                split["probe"][2] += max(0, a["pending"] - (a["words_new"] >> 32) - (a["words_new"] & 0xFFFFFFFF))
                row.update(probed_level=b["level"], probe_seconds=b["seconds"], probe_ms=b["expand_ms"])
                if b["viol_mask"]:
                    found = b
            passes.append(row)
        tr = mc.violation_trace()
        dt = time.perf_counter() - t0
        assert found["level"] == 24 and found["viol_mask"] == 1 and len(tr) == 24 and found["generated"] == E["probe_generated"]
        assert seed or E["viol_fp"] is None or found["viol_fp"] == E["viol_fp"]
        fps, _ = m.fingerprints(tr[-1][1], np.array([0, len(tr[-1][1])], dtype=np.uint64))
        assert int(fps[0]) == found["viol_fp"]                               # the reconstructed path ends in the reported violator
        if verify:
            # the reference's own golden vector against THIS run's seen-set (tests/golden/state_transfer_trace.json = the 24 states of the reference's
            # state_transfer_violation_trace.txt as packed words): state i must sit at a BFS level <= i, and its last state — level 24 is probed,
            # not inserted — must be one of the violating states the probe collected
            with open(os.path.join(ROOT, "tests", "golden", "state_transfer_trace.json")) as f:
                gt = json.load(f)
            recs = [np.array([int(w, 16) for w in st["words"]], dtype=np.uint64) for st in gt["states"]]
            gfps, _ = m.fingerprints(np.concatenate(recs), np.cumsum([0] + [len(r) for r in recs]).astype(np.uint64))
            levels = []
            for i, f_ in enumerate(gfps[:-1]):
                hit = mc.lookup(int(f_))
                assert hit is not None and 1 <= (hit[1] >> 55) <= i + 1, ("state %d of the reference trace" % (i + 1), hit)
                levels.append(int(hit[1] >> 55))
            viol = mc.probe_violators()
            assert int(gfps[-1]) in viol and viol[0] == found["viol_fp"]
            # the path THIS search took to the reference's last state (vsrmc_checker_trace_to_violator) beside the reference's own 23 steps
            path = mc.trace_to_violator(int(gfps[-1]))
            pfps, _ = m.fingerprints(np.concatenate([r for _a, r in path]), np.cumsum([0] + [len(r) for _a, r in path]).astype(np.uint64))
            ref_actions, my_actions = [st["action"] for st in gt["states"]], [a_ for a_, _r in path]
            assert len(path) == len(ref_actions) == 24 and int(pfps[-1]) == int(gfps[-1])
            S["reference_trace"] = dict(states_found_in_seen_set=len(levels), at_their_own_depth=sum(1 for i, l in enumerate(levels) if l == i + 1),
                                        last_state_among_probe_violators=True, distinct_violating_states_at_depth_24=len(viol),
                                        same_action_sequence_as_reference=my_actions == ref_actions,
                                        states_shared_with_reference=sum(1 for a_, b_ in zip(pfps, gfps) if int(a_) == int(b_)),
                                        same_action_multiset_as_reference=sorted(my_actions) == sorted(ref_actions),
                                        actions_to_the_reference_last_state=my_actions[1:], reference_actions=ref_actions[1:])
        fx = E["fx"]
        if fx.get("fp_version") == FP_VERSION and fx.get("trace") and not seed:   # the counter-example is a function of the state space alone
            S["same_trace"] = [(a_, ["%016x" % int(w) for w in rec]) for a_, rec in tr] == [(t["action"], t["words"]) for t in fx["trace"]]
        if dump_trace:                                                       # refresh of tests/golden/config3_violation.json (tools/refresh_violation_fixtures.py)
            with open(dump_trace, "w") as f:
                f.write(json.dumps(dict(trace=[dict(action=a_, words=["%016x" % int(w) for w in rec]) for a_, rec in tr])) + "\n")
        if record:
            S["alg_bytes"] += alg
            S["mat_ms"] += kms
            S["deep_ms"] += dms
            S["distinct"] += mc.distinct
            S["generated"] += gen
            S["ttfv"].append(dt)
            S["mat_s"] += t_mat
            S["n_mat"], S["mat_levels"] = n_mat, mat_levels
            S["launches"] = launches
            S["deep"] = passes
            S["split"] = split
            S["last"] = (rows, tr, mc.distinct, found["level"], found["viol_fp"])

    try:
        if seed:
            one_run(False, verify=True)
            return 0.0, S
        if not args.no_verify:
            one_run(False, verify=True)
        for _ in range(args.warmup):
            one_run(False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            one_run(True)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
    finally:
        mc.close()
    S["setup_s"] = setup
    S["oracle_levels"] = E["oracle_levels"]
    S["probe_source"] = E["probe_source"]
    return elapsed, S


def sector_granular(alg_bytes, key_accesses, kernel_s, distinct):
    """SURVEY §8(d)'s second figure: the algorithmic bytes with every 8-byte key access (one per generated successor's probe, one per insert)
    priced as the 64-byte sector it moves — 2 S + 64 g + 64 per distinct state — over the same kernel time."""
    b = alg_bytes + 56.0 * key_accesses
    achieved = b / max(kernel_s, 1e-12) / 1e9
    return {"bytes_per_state": round(b / max(1.0, distinct), 1), "achieved": round(achieved, 2), "frac": round(achieved / HBM_PEAK_GBS, 5)}


def readme_object(args, elapsed, S):
    """The README configuration's figures as JSON fields (the headline line, or the `readme` object when it is not the headline)."""
    k = args.steps
    kernel_ms = (S["mat_ms"] + S["deep_ms"]) / k
    launches = S["launches"]
    alg_run = S["alg_bytes"] / k
    avg_launch_s = kernel_ms / 1e3 / launches
    achieved = alg_run / (kernel_ms / 1e3) / 1e9
    distinct = S["distinct"] / k
    tr = committed_traffic("readme")
    return dict(
        workload="VSR.tla BFS, ReplicaCount=3 ClientCount=1 Values={v1,v2,v3} StartViewOnTimerLimit=3 (the reference README's state-transfer-"
                 "defect configuration, README:13-18 = BASELINE configs[2]), VIEW+SYMMETRY, to the first violation at depth 24: 1821858767 distinct "
                 "states, all in HBM, automatic level scheme (buffers sized from the free HBM; levels stored while the next one is predicted to fit "
                 "— here 1-%d — then virtual / streamed / probed through the seen-set alone); counter-example reconstructed in the timed region"
                 % S["mat_levels"],
        value=distinct * k / elapsed, ms_per_step=1e3 * elapsed / k, time_to_first_violation_s=round(sum(S["ttfv"]) / len(S["ttfv"]), 4),
        distinct=int(distinct), generated=int(S["generated"] / k), setup_s=round(S["setup_s"], 2), oracle_pinned_levels=S["oracle_levels"],
        violation_pinned_by=S["probe_source"], trace_equals_fixture=S["same_trace"], reference_trace_in_this_run=S.get("reference_trace"),
        sized_from_free_hbm=S["sizes"],
        roofline={"bound": "hbm", "kernel": "k_expand (all launches of a run: PLAIN instantiation for the stored levels and the sub-slices of a streamed level, one-mode instantiations for the virtual / regenerated / probed passes)",
                  "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
                  "traffic": tr["bytes_per_launch"], "traffic_source": tr["source"],
                  "avg_launch_ms": round(1e3 * avg_launch_s, 4), "launches": launches, "alg_bytes_per_launch": round(alg_run / launches),
                  "B_alg_per_state": round(alg_run / distinct, 1),
                  "sector_granular": sector_granular(alg_run, S["generated"] / k + distinct, kernel_ms / 1e3, distinct),
                  "kernel_ms_per_step": {"k_expand": round(kernel_ms, 3), "k_expand_materialised_levels": round(S["mat_ms"] / k, 3),
                                         "k_expand_deep_passes": round(S["deep_ms"] / k, 3)},
                  # the same roofline per KIND of pass = per instantiation of k_expand (one run, the last timed one): stored levels <313,1>, the virtual
                  # level <313,4>, its regeneration from the claim bitmap <313,3>, the level inserted beyond the buffers <313,1> into scratch, the probe <313,6> (+ k_probe_resolve; <313,2> when a violation has been seen or a limit is re-checked)
                  "per_pass": {name: {"kernel_ms": round(v[0], 3), "launches": int(v[2]), "alg_bytes": round(v[1]),
                                      "achieved": round(v[1] / max(v[0] / 1e3, 1e-12) / 1e9, 2), "frac": round(v[1] / max(v[0] / 1e3, 1e-12) / 1e9 / HBM_PEAK_GBS, 5)}
                               for name, v in S.get("split", {}).items() if v[0] > 0}},
        materialised=dict(levels=S["mat_levels"], distinct=S["n_mat"], seconds=round(S["mat_s"] / k, 4), states_per_s=round(S["n_mat"] / (S["mat_s"] / k), 1)),
        deep_passes=[{k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in row.items()} for row in S["deep"]])


def config2_object(args, elapsed, S):
    """BASELINE configs[1] (the shipped VSR.cfg constants) as JSON fields: the headline of rounds 1-2, now the `config2` object."""
    value = S["distinct"] / elapsed
    avg_launch_s = S["expand_ms"] / 1e3 / max(1, S["launches"])
    achieved = S["alg_bytes"] / max(1, S["launches"]) / avg_launch_s / 1e9
    g = S["generated"] / S["distinct"]
    s_bytes = 8.0 * S["words"] / S["distinct"]
    tr = committed_traffic("config2")
    return dict(
        workload="VSR.tla BFS, ReplicaCount=3 ClientCount=1 Values={v1,v2} StartViewOnTimerLimit=2 (BASELINE configs[1] = shipped VSR.cfg), "
                 "VIEW+SYMMETRY, to first violation: 28 levels, 319228361 distinct states; every level asserted against the CPU oracle's fixture",
        value=value, ms_per_step=1e3 * elapsed / args.steps, time_to_first_violation_s=round(sum(S["ttfv"]) / len(S["ttfv"]), 4),
        generated_per_distinct=round(g, 3), record_bytes=round(s_bytes, 1), table_slots_log2=TABLE_LOG2,
        roofline={"bound": "hbm", "kernel": "k_expand", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                  "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": tr["bytes_per_launch"], "traffic_source": tr["source"],
                  "avg_launch_ms": round(1e3 * avg_launch_s, 4), "launches": S["launches"] // args.steps,
                  "alg_bytes_per_launch": round(S["alg_bytes"] / max(1, S["launches"])), "B_alg_per_state": round(2 * s_bytes + 8 * g + 8, 1),
                  "sector_granular": sector_granular(S["alg_bytes"], S["generated"] + S["distinct"], S["expand_ms"] / 1e3, S["distinct"]),
                  "kernel_ms_per_step": {"k_expand": round(S["expand_ms"] / args.steps, 3)}})


def collision_estimate(n):
    """TLC prints, at the end of every run, the probability that two distinct states shared a 64-bit fingerprint (a false merge drops
    a state silently).  This is the birthday bound n^2 / 2^65 for n distinct states; TLC's own "calculated (optimistic)" figure,
    d * (g - d) / 2^64 for d distinct of g generated states, is reported beside it."""
    return float(n) * float(n) / 2.0 ** 65


def run_config4(args):
    """BASELINE configs[3] (ReplicaCount=3, ClientCount=2, Values={v1,v2,v3}, StartViewOnTimerLimit=3) under the documented policy for VSR.tla:421
    (`assume_commit_number`: strict TLC semantics abort at that line after 5 states, tests/test_gpu_parity.py) as deep as the CPU oracle's fixture
    goes (tests/golden/oracle_levels_config4.json): one verified run (every level figure, per-action counts, fingerprint checksums), then the
    timed ones.  No violation within that depth; the object is a rate, not a time-to-violation.  -> JSON fields"""
    import torch
    import vsr_tlaplus_amd as vt
    torch.cuda.set_device(0)
    with open(os.path.join(ROOT, "tests", "golden", "oracle_levels_config4.json")) as f:
        g = json.load(f)
    p = g["params"]
    m = vt.Model.from_constants(R=p["R"], C_=p["C"], n=p["n"], L=p["L"], symmetry=p["symmetry"], invariant_mask=p["inv_mask"], assume_commit_number=True)
    mc = vt.ModelChecker.auto(m, device=0)
    last = g["levels"][-1]["level"]
    sums = g.get("fp_version") == FP_VERSION

    def one_run(verify):
        mc.reset()
        t0 = time.perf_counter()
        kms, stored = 0.0, 1
        while mc.depth < last:
            kind, a, b = mc.advance()
            lv = g["levels"][a["level"] - 1]
            assert (a["n_new"], a["generated"], a["deadlocks"], a["max_bag"], a["viol_mask"]) == (lv["new"], lv["generated"], lv["deadlocks"], lv["max_bag"], 0), a["level"]
            kms += a["expand_ms"] + a["materialize_ms"] + (b["expand_ms"] if b is not None else 0.0)
            stored += kind == "level"
            if verify:
                assert [int(x) for x in a["act_generated"][1:16]] == lv["act_generated"][1:16], a["level"]
                x, s_ = (mc.level_checksum()[:2]) if kind == "level" else (a["fp_xor"], a["fp_sum"])
                assert not sums or ("%016x" % x, "%016x" % s_) == (lv["fp_xor"], lv["fp_sum"]), a["level"]
        assert mc.distinct == g["distinct"] and mc.violation is None
        return time.perf_counter() - t0, kms, stored

    try:
        if not args.no_verify:
            one_run(True)
        k = max(1, min(args.steps, 3))
        one_run(False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = [one_run(False) for _ in range(k)]
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
    finally:
        mc.close()
    return dict(workload="VSR.tla BFS, ReplicaCount=3 ClientCount=2 Values={v1,v2,v3} StartViewOnTimerLimit=3 (BASELINE configs[3]) under the documented policy "
                         "assume_commit_number for VSR.tla:421 (strict TLC semantics abort there), VIEW+SYMMETRY, the %d levels the CPU oracle's fixture holds: "
                         "%d distinct states, no violation; every level asserted" % (last, g["distinct"]),
                value=round(g["distinct"] * k / elapsed, 1), unit="distinct states/s", steps=k, ms_per_step=round(1e3 * elapsed / k, 3), depth=last,
                distinct=g["distinct"], oracle_pinned_levels=len(g["levels"]), stored_levels=rows[-1][2], k_expand_ms_per_step=round(sum(r[1] for r in rows) / k, 3))


def run_config5(args):
    """BASELINE configs[4] (ReplicaCount=5, ClientCount=1, Values={v1,v2}, StartViewOnTimerLimit=2: the "288 GB/GPU FPSet sizing stress") on this ONE GPU as
    deep as its HBM goes, through the automatic level scheme: every level the CPU oracle's fixture holds (tests/golden/oracle_levels_config5.json: 14 levels,
    3 177 730 826 states) asserted — new states, successors in total and per action, deadlocks, largest bag, fingerprint checksums — then the probe of the
    level after it (no CPU counterpart: 3.7e10 successors; GPU-sourced, labelled so), and the whole run once more under the audit seed.  Neither a violation
    nor exhaustion is within one GPU's reach: the object is a rate and a depth, not a time-to-violation.  -> JSON fields"""
    import torch
    import vsr_tlaplus_amd as vt
    torch.cuda.set_device(0)
    with open(os.path.join(ROOT, "tests", "golden", "oracle_levels_config5.json")) as f:
        g = json.load(f)
    p = g["params"]
    last = g["levels"][-1]["level"]
    sums = g.get("fp_version") == FP_VERSION

    def one(seed):
        m = vt.Model.from_constants(R=p["R"], C_=p["C"], n=p["n"], L=p["L"])
        if seed:
            m.set_fp_seed(seed)
        mc = vt.ModelChecker.auto(m, device=0)
        try:
            t0 = time.perf_counter()
            kms, stored, probed = 0.0, 1, None
            while mc.depth < last:
                kind, a, b = mc.advance()
                lv = g["levels"][a["level"] - 1]
                assert (a["n_new"], a["generated"], a["deadlocks"], a["max_bag"], a["viol_mask"]) == (lv["new"], lv["generated"], lv["deadlocks"], lv["max_bag"], 0), a["level"]
                assert [int(x) for x in a["act_generated"][1:16]] == lv["act_generated"][1:16], a["level"]
                if sums and not seed:
                    x, s_ = (mc.level_checksum()[:2]) if kind == "level" else (a["fp_xor"], a["fp_sum"])
                    assert ("%016x" % x, "%016x" % s_) == (lv["fp_xor"], lv["fp_sum"]), a["level"]
                kms += a["expand_ms"] + a["materialize_ms"] + (b["expand_ms"] if b is not None else 0.0)
                stored += kind == "level"
                if b is not None:
                    probed = dict(level=b["level"], generated=b["generated"], deadlocks=b["deadlocks"], viol_mask=b["viol_mask"], seconds=round(b["seconds"], 3))
            dt = time.perf_counter() - t0
            assert mc.distinct == sum(lv["new"] for lv in g["levels"]) and mc.violation is None
            return dict(seconds=dt, kernel_ms=kms, stored_levels=stored, probed=probed, distinct=mc.distinct,
                        table_log2=int(mc.options.table_log2), load=round(mc.distinct / float(1 << int(mc.options.table_log2)), 3))
        finally:
            mc.close()

    r0 = one(0)
    r1 = one(AUDIT_SEED) if not args.no_verify else None
    same = None if r1 is None else (r1["probed"] is not None and r0["probed"] is not None and
                                    (r1["probed"]["level"], r1["probed"]["generated"], r1["probed"]["deadlocks"], r1["probed"]["viol_mask"]) ==
                                    (r0["probed"]["level"], r0["probed"]["generated"], r0["probed"]["deadlocks"], r0["probed"]["viol_mask"]))
    return dict(workload="VSR.tla BFS, ReplicaCount=5 ClientCount=1 Values={v1,v2} StartViewOnTimerLimit=2 (BASELINE configs[4], the FPSet sizing stress), VIEW+SYMMETRY, "
                         "the %d levels the CPU oracle's fixture holds: %d distinct states, no violation; every level asserted; the level after them probed "
                         "(GPU-sourced: no CPU counterpart)" % (last, r0["distinct"]),
                value=round(r0["distinct"] / r0["seconds"], 1), unit="distinct states/s", steps=1, ms_per_step=round(1e3 * r0["seconds"], 3), depth=last,
                distinct=r0["distinct"], oracle_pinned_levels=len(g["levels"]), stored_levels=r0["stored_levels"], k_expand_ms_per_step=round(r0["kernel_ms"], 3),
                seen_set=dict(slots_log2=r0["table_log2"], load=r0["load"]), probed=r0["probed"], probed_source="gpu",
                second_seed=None if r1 is None else dict(seed=hex(AUDIT_SEED), every_level_equal_to_the_fixture=True, probed=r1["probed"], probe_figures_equal=same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-verify", action="store_true", help="skip the untimed verification runs (profiling: one run = the kernel launches of one BFS)")
    ap.add_argument("--no-config3", action="store_true", help="skip the README configuration (takes the whole HBM): config 2 is the headline")
    ap.add_argument("--no-config2", action="store_true", help="skip the config-2 object")
    ap.add_argument("--no-config4", action="store_true", help="skip the config-4 object (BASELINE configs[3] under assume_commit_number)")
    ap.add_argument("--no-config5", action="store_true", help="skip the config-5 object (BASELINE configs[4]: 14 oracle-pinned levels + the probe of level 15, two seeds)")
    ap.add_argument("--workload", choices=["auto", "readme", "config3", "config2"], default="auto",
                    help="auto (default): the README defect configuration (BASELINE configs[2], fits one MI355X) is the headline and, with "
                         "--full, config 2 (BASELINE configs[1]) an object beside it; readme / config3: only the former; config2: only the latter")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline does not need: the untimed verification run and the second-hash audit, the "
                         "config2 / config4 / config5 objects, the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed run computed as DIR/<name>.npy (float64; N = 1)")
    args = ap.parse_args()
    if not args.full:                                                        # a plain run: the headline alone
        args.no_verify = args.no_cpu_baseline = True
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 or world > 1 or os.environ.get("VSR_BENCH_SHARDED"):   # VSR_BENCH_SHARDED=1: the N > 1 leg on one rank
        if args.dump_outputs:
            raise SystemExit("--dump-outputs: the N = 1 leg only")
        from vsr_tlaplus_amd import sharded_bench
        return sharded_bench.main(args, sys.modules[__name__])
    want_readme = args.workload in ("auto", "readme", "config3") and not args.no_config3
    want_c2 = args.workload in ("auto", "config2") and not args.no_config2 and (args.full or not want_readme)
    c2 = rd = c4 = c5 = None
    audit = None
    if want_c2:
        elapsed, S, _ = run_single(args)
        c2 = config2_object(args, elapsed, S)
        last = S["last"]
    if want_readme:
        # a README leg that cannot run (e.g. another process holds the HBM) is an ERROR of the bench, not a reason to print another workload's
        # number under the headline: the exception propagates and the exit code is not 0
        elapsed, S = run_readme(args, os.environ.get("VSR_BENCH_DUMP_TRACE"))
        rd = readme_object(args, elapsed, S)
        last = S["last"]
    if args.dump_outputs:                                                    # the headline's last timed run
        dump_outputs(run_outputs(*last), args.dump_outputs)
    if args.full and args.workload == "auto" and not args.no_config4 and not args.no_config3:
        c4 = run_config4(args)
    if args.full and args.workload == "auto" and not args.no_config5 and not args.no_config3:
        c5 = run_config5(args)
    if not args.no_verify:
        # second-hash audit: the untimed verification runs once more under another member of the fingerprint family — every per-level count
        # (new states, generated, deadlocks, largest bag, per action) is asserted against the same oracle fixtures inside the runs
        done = []
        if want_c2:
            run_single(args, seed=AUDIT_SEED)
            done.append("config2")
        if want_readme:
            run_readme(args, seed=AUDIT_SEED)
            done.append("readme")
        audit = {"seeds": ["0x0", hex(AUDIT_SEED)], "equal": True, "workloads": done,
                 "note": "every level's new / generated / deadlocks / largest bag / per-action counts equal the CPU oracle's fixture under both "
                         "fingerprint functions (vsrmc_model_set_fp_seed): a 64-bit collision under one would have to repeat under the other"}
    head = rd if rd is not None else c2
    cfg = README if rd is not None else CONFIG
    out = {
        "metric": "distinct states/sec (whole node) + time-to-first-violation, VSR 3-replica", "value": round(head["value"], 1),
        "unit": "distinct states/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(head["ms_per_step"], 3),
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u64", "data": "synthetic",
        "config": {"workload": head["workload"], "trace": "predecessor pointers in the seen-set, counter-example reconstructed in the timed region"},
        "time_to_first_violation_s": head["time_to_first_violation_s"],
        "roofline": head["roofline"],
    }
    for k_, v in head.items():
        if k_ not in ("workload", "value", "ms_per_step", "time_to_first_violation_s", "roofline"):
            out[k_] = v
    n_states = head.get("distinct", EXPECT["distinct"])
    n_gen = head.get("generated", sum(lv["generated"] for lv in EXPECT["levels"]))
    out["fingerprint_collision_estimate"] = {"n2_over_2_65": collision_estimate(n_states), "tlc_optimistic": float(n_states) * float(max(0, n_gen - n_states)) / 2.0 ** 64,
                                             "distinct": n_states, "generated": n_gen,
                                             "note": "expected number of 64-bit fingerprint collisions among the distinct states (birthday bound n^2 / 2^65) and TLC's own "
                                                     "'calculated (optimistic)' figure d * (g - d) / 2^64 (every successor judged seen could be one; the CLI prints the same): "
                                                     "a false merge would drop a state silently — what collision_audit (a second hash) is for"}
    if rd is not None and c2 is not None:
        c2["value"] = round(c2["value"], 1)
        c2["ms_per_step"] = round(c2["ms_per_step"], 3)
        out["config2"] = c2
    if c4 is not None:
        out["config4"] = c4
    if c5 is not None:
        out["config5"] = c5
    out["collision_audit"] = audit
    if not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args.cpu_seconds, cfg)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
