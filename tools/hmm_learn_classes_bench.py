"""Measures class-batched HMM training against a loop of single-class trainings on one GPU; prints one
JSON record (optionally also written to --out).

For each N (default 5, 64, 70): K = 20 classes, each with its own random model (e2vq_hmm_init type 3) with M = 1024 and
S = 200 sequences of T = 300 symbols drawn around a class-specific ramp.  Every training runs exactly --iters E-steps
(val_auto = -inf, max_iterations = --iters):
  batched  e2vq_hmm_train_classes over the K classes (the grid batch of one (N, M)): per iteration one k_hmm_fb_grid launch
           (N <= 64; above, one k_hmm_fb_wg launch per class), one copy back, one k_hmm_reestimate_grid / k_hmm_adjustb_grid
  loop     e2vq_hmm_train once per class, one class after the other, in the same warm process
Wall times: --warmup + --reps calls of each in a plain run (no tracer), the median of the timed calls.  Kernel times: a
`rocprofv3 --kernel-trace` run of its own (the same calls); every k_hmm_* launch of a call is summed, the warm-up calls
dropped, the median over the calls reported.  `speedup` is loop / batched.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WAVE_N = 64


def workload(N, M, K, S, T, seed=2026):
    import numpy as np

    import ecoz2rs_amd as e

    e.hmm.set_random_seed(seed + N)
    models = [e.hmm.init_model(N, M, 3) for _ in range(K)]
    rng = np.random.default_rng(seed)
    classes = []
    for k in range(K):
        ramp = np.linspace(0, M - 1, T)
        classes.append([np.clip((ramp * (0.5 + k / (2 * K)) + rng.normal(0, M / 16, T)).round(), 0, M - 1).astype(np.uint16)
                        for _ in range(S)])
    return models, classes


def calls_of(args):
    import ecoz2rs_amd as e

    models, classes = workload(args.n, args.m, args.k, args.s, args.t)
    va, it = float("-inf"), args.iters
    return {
        "batched": lambda: e.hmm.train_classes(models, classes, 1e-5, va, it),
        "loop": lambda: [e.hmm.train(*m, c, 1e-5, va, it) for m, c in zip(models, classes)],
    }


def run(args):
    """the measured calls (plain, or under rocprofv3); prints the wall times as JSON"""
    wall = {}
    for kind, fn in calls_of(args).items():  # (one kind after the other: the trace is cut by launch counts)
        ts = []
        for _ in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        wall[kind] = dict(median_ms=statistics.median(ts[args.warmup:]) * 1e3, all_ms=[round(x * 1e3, 3) for x in ts])
    print(json.dumps(wall))


def launches_per_call(N, K, iters):
    """k_hmm_* launches of one call with epsilon > 0 and exactly `iters` E-steps per class"""
    batched = iters * ((1 if N <= WAVE_N else K) + 2)
    return dict(batched=batched, loop=K * iters * 3)


def kernel_ms(trace, per, calls, warmup):
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(trace))
                  if "k_hmm_" in r["Kernel_Name"])
    want = sum(per.values()) * calls
    if len(rows) != want:
        return dict(error=f"{len(rows)} k_hmm_ launches, expected {want}")
    out, at = {}, 0
    for kind in ("batched", "loop"):  # (run() calls the kinds in this order)
        sel = rows[at:at + per[kind] * calls]
        at += per[kind] * calls
        sums = [sum(b - a for a, b, _ in sel[c * per[kind]:(c + 1) * per[kind]]) / 1e6 for c in range(calls)]
        out[kind] = dict(kernel_ms=statistics.median(sums[warmup:]), launches_per_call=per[kind],
                         kernels=sorted({n.split("(")[0].replace("void ", "") for _, _, n in sel}))
    return out


def child(args, N, extra=()):
    return [*extra, sys.executable, os.path.abspath(__file__), "--run", "--n", str(N), "--m", str(args.m), "--k", str(args.k),
            "--s", str(args.s), "--t", str(args.t), "--iters", str(args.iters), "--reps", str(args.reps),
            "--warmup", str(args.warmup)]


def last_json(r, what):
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{what}: failed with status {r.returncode}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true", help="(internal) the measured calls")
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--ns", default="5,64,70")
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--s", type=int, default=200)
    ap.add_argument("--t", type=int, default=300)
    ap.add_argument("--iters", type=int, default=10, help="E-steps per class (-I)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child run")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.run:
        return run(args)
    rec = dict(tool="tools/hmm_learn_classes_bench.py", K=args.k, S_per_class=args.s, T=args.t, M=args.m, iters=args.iters,
               reps=args.reps, warmup=args.warmup, by_N={})
    calls = args.warmup + args.reps
    for N in [int(x) for x in args.ns.split(",")]:
        wall = last_json(subprocess.run(child(args, N), capture_output=True, text=True, timeout=args.timeout, cwd=ROOT),
                         f"N = {N}: wall run")
        with tempfile.TemporaryDirectory() as d:
            r = subprocess.run(child(args, N, ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"]),
                               capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
            last_json(r, f"N = {N}: rocprofv3 run")
            traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            if len(traces) != 1:
                raise SystemExit(f"N = {N}: expected one kernel trace, found {traces}")
            k = kernel_ms(traces[0], launches_per_call(N, args.k, args.iters), calls, args.warmup)
        ent = dict(wall_ms={kind: wall[kind]["median_ms"] for kind in wall}, wall_all_ms={kind: wall[kind]["all_ms"] for kind in wall},
                   kernels=k)
        ent["speedup_wall"] = wall["loop"]["median_ms"] / wall["batched"]["median_ms"]
        if "batched" in k:
            ent["speedup_kernel"] = k["loop"]["kernel_ms"] / k["batched"]["kernel_ms"]
        rec["by_N"][str(N)] = ent
        print(json.dumps({N: ent}), file=sys.stderr)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
