"""Measures HMM Viterbi decoding against forward scoring on one GPU; prints one JSON record
(optionally also written to --out).

For each N (default 5, 64, 141): one random model (e2vq_hmm_init type 0) with M = 1024 and S = 4096 sequences of
T = 300 random symbols.  The same sequences go through
  viterbi        e2vq_hmm_viterbi with the path: k_hmm_viterbi<true> (N <= 64) / k_hmm_viterbi_wg<true>, then k_hmm_backtrack
  viterbi_nopath e2vq_hmm_viterbi without the path: the <false> instantiation alone
  score          e2vq_hmm_score under the one model: k_hmm_score / k_hmm_score_wg
--warmup + --reps calls of each.  Kernel times come from a `rocprofv3 --kernel-trace` run of this script (--run) per N:
the launches of one call are summed (several launches when the back-pointer table is cut into chunks), the warm-up
calls dropped, and the median over the calls reported; `ratio` is viterbi / score (the target: <= 1.5 at N = 5 and 64).
Wall times of the whole calls (host logarithms, uploads, copies back included) come from the same run.
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
    "viterbi": re.compile(r"k_hmm_viterbi(_wg)?<true>|k_hmm_backtrack"),
    "viterbi_nopath": re.compile(r"k_hmm_viterbi(_wg)?<false>"),
    "score": re.compile(r"k_hmm_score(_wg)?\("),
}


def workload(N, M, S, T, seed=2026):
    import numpy as np

    import ecoz2rs_amd as e

    e.hmm.set_random_seed(seed + N)
    model = e.hmm.init_model(N, M, 0)
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(0, M, T).astype(np.uint16) for _ in range(S)]
    return model, seqs


def run(args):
    """the measured calls (under rocprofv3); prints the wall times as JSON"""
    import ecoz2rs_amd as e

    (pi, A, B), seqs = workload(args.n, args.m, args.s, args.t)
    calls = {
        "viterbi": lambda: e.hmm.viterbi(pi, A, B, seqs),
        "viterbi_nopath": lambda: e.hmm.viterbi(pi, A, B, seqs, want_path=False),
        "score": lambda: e.hmm.score([(pi, A, B)], seqs),
    }
    wall = {}
    for kind, fn in calls.items():  # (one kind after the other: the trace is split by kernel name)
        ts = []
        for _ in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        wall[kind] = statistics.median(ts[args.warmup:]) * 1e3
    print(json.dumps(wall))


def kernel_ms(trace, calls, warmup):
    rows = list(csv.DictReader(open(trace)))
    out = {}
    for kind, rx in KINDS.items():
        sel = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows if rx.search(r["Kernel_Name"]))
        if not sel or len(sel) % calls:
            out[kind] = dict(error=f"{len(sel)} launches for {calls} calls")
            continue
        per = len(sel) // calls
        sums = [sum(b - a for a, b, _ in sel[c * per:(c + 1) * per]) / 1e6 for c in range(calls)]
        out[kind] = dict(kernel_ms=statistics.median(sums[warmup:]), launches_per_call=per,
                         kernels=sorted({n.split("(")[0].replace("void ", "") for _, _, n in sel}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true", help="(internal) the measured calls, for rocprofv3")
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--ns", default="5,64,141")
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--s", type=int, default=4096)
    ap.add_argument("--t", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.run:
        return run(args)
    rec = dict(tool="tools/hmm_viterbi_bench.py", M=args.m, S=args.s, T=args.t, reps=args.reps, warmup=args.warmup, by_N={})
    for N in [int(x) for x in args.ns.split(",")]:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--",
                   sys.executable, os.path.abspath(__file__), "--run", "--n", str(N), "--m", str(args.m), "--s", str(args.s),
                   "--t", str(args.t), "--reps", str(args.reps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"N = {N}: rocprofv3 run failed with status {r.returncode}")
            wall = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            if len(traces) != 1:
                raise SystemExit(f"N = {N}: expected one kernel trace, found {traces}")
            k = kernel_ms(traces[0], args.warmup + args.reps, args.warmup)
        for kind in k:
            k[kind]["call_wall_ms"] = wall[kind]
        ent = dict(kinds=k)
        if "kernel_ms" in k["viterbi"] and "kernel_ms" in k["score"]:
            ent["ratio"] = k["viterbi"]["kernel_ms"] / k["score"]["kernel_ms"]
            ent["ratio_nopath"] = k["viterbi_nopath"]["kernel_ms"] / k["score"]["kernel_ms"]
            ent["symbols_per_s_viterbi"] = args.s * args.t / (k["viterbi"]["kernel_ms"] * 1e-3)
        rec["by_N"][str(N)] = ent
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
