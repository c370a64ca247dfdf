"""Measures `hmm segment` against what the commit before it could do with the same models and stream;
prints one JSON record (optionally also written to --out).

One stream of --t random symbols (default 38 265), M = 1024, K = 20 random models (e2vq_hmm_init type 0) of N states each,
ln_switch = -5.  Per N (default 5, 16, 32, 64):
  segment     one e2vq_hmm_segment call: k_hmm_segment + k_hmm_segment_backtrack
  comparator  K e2vq_hmm_viterbi calls with the path on the same stream, one model each (k_hmm_viterbi<true> +
              k_hmm_backtrack), kernel times summed: the same in-class additions without the coupling between classes
--warmup + --reps of each.  Kernel times come from one `rocprofv3 --kernel-trace` run of this script (--run) per N; the
segment call's own HIP-event time (e2vq_hmm_segment_last_kernel_ms) is recorded next to it.  median and min .. max over the
repetitions; `ratio` = comparator / segment of the medians (> 1: segment is faster).  Wall times of the whole calls come
from the same run.  --files: additionally the wall time of `ecoz2 hmm segment --sequences` against `ecoz2 hmm scan
--sequences --window 100 --hop 1` on the stream written as a .seq (they compute different things; for context only).
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = {
    "segment": re.compile(r"k_hmm_segment"),
    "comparator": re.compile(r"k_hmm_viterbi(_wg)?<true>|k_hmm_backtrack"),
}


def workload(N, M, K, T, seed=2026):
    import numpy as np

    import ecoz2rs_amd as e

    e.hmm.set_random_seed(seed + N)
    models = [e.hmm.init_model(N, M, 0) for _ in range(K)]
    sym = np.random.default_rng(seed).integers(0, M, T).astype(np.uint16)
    return models, sym


def run(args):
    """the measured calls (under rocprofv3); prints wall and HIP-event times as JSON"""
    import numpy as np

    import ecoz2rs_amd as e

    models, sym = workload(args.n, args.m, args.k, args.t)
    offs = np.array([0, len(sym)], dtype=np.int64)
    out = {}
    ts, ev = [], []
    for _ in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        e.hmm.segment(models, sym, offs, args.ln_switch)
        ts.append((time.perf_counter() - t0) * 1e3)
        ev.append(e.hmm.segment_last_kernel_ms())
    out["segment"] = dict(call_wall_ms=statistics.median(ts[args.warmup:]), event_ms=statistics.median(ev[args.warmup:]),
                          event_ms_min=min(ev[args.warmup:]), event_ms_max=max(ev[args.warmup:]))
    ts = []
    for _ in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        for m in models:
            e.hmm.viterbi(*m, [sym])
        ts.append((time.perf_counter() - t0) * 1e3)
    out["comparator"] = dict(call_wall_ms=statistics.median(ts[args.warmup:]))
    print(json.dumps(out))


def kernel_ms(trace, calls, warmup):
    rows = list(csv.DictReader(open(trace)))
    out = {}
    for kind, rx in KINDS.items():
        sel = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows if rx.search(r["Kernel_Name"]))
        if not sel or len(sel) % calls:
            out[kind] = dict(error=f"{len(sel)} launches for {calls} calls")
            continue
        per = len(sel) // calls
        sums = [sum(b - a for a, b, _ in sel[c * per:(c + 1) * per]) / 1e6 for c in range(calls)][warmup:]
        out[kind] = dict(kernel_ms=statistics.median(sums), kernel_ms_min=min(sums), kernel_ms_max=max(sums), launches_per_call=per,
                         kernels=sorted({n.split("(")[0].replace("void ", "") for _, _, n in sel}))
    return out


def files_wall(args, N):
    """wall ms of the two commands on the stream as a .seq"""
    import ecoz2rs_amd as e

    exe = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
    models, sym = workload(N, args.m, args.k, args.t)
    with tempfile.TemporaryDirectory() as d:
        for k, m in enumerate(models):
            e.hmm.save_model(os.path.join(d, "hmms", f"c{k:02d}.hmm"), f"c{k:02d}", *m)
        os.makedirs(os.path.join(d, "seq"))
        e.formats.write_seq(os.path.join(d, "seq", "x.seq"), "x", args.m, sym)
        out = {}
        for name, extra in (("hmm_segment", ["segment", "--switch-penalty", str(args.ln_switch)]),
                            ("hmm_scan_hop1", ["scan", "--window", "100", "--hop", "1"])):
            t0 = time.perf_counter()
            r = subprocess.run([exe, "hmm", *extra, "--models", "hmms", "-c", name, "--sequences", "seq/x.seq"], cwd=d,
                               capture_output=True, text=True, timeout=args.timeout)
            out[name + "_wall_ms"] = (time.perf_counter() - t0) * 1e3
            if r.returncode != 0:
                raise SystemExit(f"{name}: exit {r.returncode}: {r.stdout[-2000:]}{r.stderr[-2000:]}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true", help="(internal) the measured calls, for rocprofv3")
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--ns", default="5,16,32,64")
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--t", type=int, default=38265)
    ap.add_argument("--ln-switch", type=float, default=-5.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--files", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.run:
        return run(args)
    rec = dict(tool="tools/hmm_segment_bench.py", M=args.m, K=args.k, T=args.t, ln_switch=args.ln_switch, reps=args.reps,
               warmup=args.warmup, by_N={})
    for N in [int(x) for x in args.ns.split(",")]:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--",
                   sys.executable, os.path.abspath(__file__), "--run", "--n", str(N), "--m", str(args.m), "--k", str(args.k),
                   "--t", str(args.t), "--ln-switch", str(args.ln_switch), "--reps", str(args.reps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"N = {N}: rocprofv3 run failed with status {r.returncode}")
            host = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            if len(traces) != 1:
                raise SystemExit(f"N = {N}: expected one kernel trace, found {traces}")
            k = kernel_ms(traces[0], args.warmup + args.reps, args.warmup)
        for kind in k:
            k[kind].update(host[kind])
        ent = dict(kinds=k)
        if "kernel_ms" in k["segment"] and "kernel_ms" in k["comparator"]:
            ent["ratio"] = k["comparator"]["kernel_ms"] / k["segment"]["kernel_ms"]
            ent["ratio_wall"] = k["comparator"]["call_wall_ms"] / k["segment"]["call_wall_ms"]
        if args.files:
            ent["files"] = files_wall(args, N)
        rec["by_N"][str(N)] = ent
        print(json.dumps({str(N): ent}), flush=True)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
