"""Measures grid-batched HMM training against a loop of class-batched trainings on one GPU; prints one
JSON record (optionally also written to --out).

Workload: K = 20 classes, S = 200 sequences of T = 300 symbols per class and codebook size (drawn around a
class-specific ramp), one random model (e2vq_hmm_init type 3) per (N, M, class), over the grid N in --ns x M in --ms
(default {5, 16, 64} x {64, 128, 256, 512, 1024}).  Every training runs exactly --iters E-steps (val_auto = -inf,
max_iterations = --iters).  Shapes: each N alone over all M, and the whole grid.  Per shape:
  grid   one e2vq_hmm_train_grid call over every (N, M, class) of the shape (the default ECOZ2_HMM_LEARN_BATCH_BYTES)
  loop   e2vq_hmm_train_classes once per (N, M) of the shape, one after the other, in the same warm process
Wall times: --warmup + --reps calls of each in a plain run (no tracer), the median of the timed calls.  Kernel times: a
`rocprofv3 --kernel-trace` run of its own (the same calls); the grid's launches are the k_hmm_*_grid kernels, the loop's
the k_hmm_*_classes ones, each cut into calls by its launch count per call, the warm-up calls dropped, the median over the
calls reported.  `speedup` is loop / grid.
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


def workload(Ns, Ms, K, S, T, seed=2026):
    """-> models [(pi, A, B)] in grid order, the shared sequences, each model's range, and the (N, M) of each model"""
    import numpy as np

    import ecoz2rs_amd as e

    rng = np.random.default_rng(seed)
    seqs, cls_range = [], {}
    for M in Ms:
        ramp = np.linspace(0, M - 1, T)
        for k in range(K):
            lo = len(seqs)
            seqs += [np.clip((ramp * (0.5 + k / (2 * K)) + rng.normal(0, M / 16, T)).round(), 0, M - 1).astype(np.uint16)
                     for _ in range(S)]
            cls_range[(M, k)] = (lo, len(seqs))
    models, ranges, points = [], [], []
    for N in Ns:
        for M in Ms:
            e.hmm.set_random_seed(seed + N + M)
            for k in range(K):
                models.append(e.hmm.init_model(N, M, 3))
                ranges.append(cls_range[(M, k)])
                points.append((N, M))
    return models, seqs, ranges, points


def calls_of(args):
    import ecoz2rs_amd as e

    Ns, Ms = [int(x) for x in args.ns.split(",")], [int(x) for x in args.ms.split(",")]
    models, seqs, ranges, points = workload(Ns, Ms, args.k, args.s, args.t)
    va, it = float("-inf"), args.iters
    per_point = []
    for i in range(0, len(models), args.k):  # (K models of one (N, M), their classes' sequences)
        per_point.append((models[i:i + args.k], [seqs[lo:hi] for lo, hi in ranges[i:i + args.k]]))
    return {
        "grid": lambda: e.hmm.train_grid(models, seqs, ranges, 1e-5, va, it),
        "loop": lambda: [e.hmm.train_classes(ms, cs, 1e-5, va, it) for ms, cs in per_point],
    }


def run(args):
    """the measured calls (plain, or under rocprofv3); prints the wall times as JSON"""
    wall = {}
    for kind, fn in calls_of(args).items():
        ts = []
        for _ in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        wall[kind] = dict(median_ms=statistics.median(ts[args.warmup:]) * 1e3, all_ms=[round(x * 1e3, 3) for x in ts])
    print(json.dumps(wall))


def kernel_ms(trace, calls, warmup):
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(trace))
                  if "k_hmm_" in r["Kernel_Name"])
    out = {}
    for kind, tag in (("grid", "_grid"), ("loop", "_classes")):
        sel = [r for r in rows if tag in r[2].split("(")[0]]
        if not sel or len(sel) % calls:
            return dict(error=f"{kind}: {len(sel)} launches, not a multiple of {calls} calls")
        per = len(sel) // calls
        sums = [sum(b - a for a, b, _ in sel[c * per:(c + 1) * per]) / 1e6 for c in range(calls)]
        out[kind] = dict(kernel_ms=statistics.median(sums[warmup:]), launches_per_call=per,
                         kernels=sorted({n.split("(")[0].replace("void ", "") for _, _, n in sel}))
    if len(rows) != sum(out[k]["launches_per_call"] for k in out) * calls:
        return dict(error=f"{len(rows)} k_hmm_ launches in all: other kernels than the grid's and the loop's")
    return out


def child(args, ns, extra=()):
    return [*extra, sys.executable, os.path.abspath(__file__), "--run", "--ns", ns, "--ms", args.ms, "--k", str(args.k),
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
    ap.add_argument("--ns", default="5,16,64")
    ap.add_argument("--ms", default="64,128,256,512,1024")
    ap.add_argument("--shapes", default=None, help="';'-separated N lists (default: each N alone, then all of --ns)")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--s", type=int, default=200)
    ap.add_argument("--t", type=int, default=300)
    ap.add_argument("--iters", type=int, default=10, help="E-steps per model (-I)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child run")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.run:
        return run(args)
    shapes = args.shapes.split(";") if args.shapes else args.ns.split(",") + [args.ns]
    rec = dict(tool="tools/hmm_learn_grid_bench.py", K=args.k, S_per_class=args.s, T=args.t, Ms=args.ms, iters=args.iters,
               reps=args.reps, warmup=args.warmup, batch_bytes=os.environ.get("ECOZ2_HMM_LEARN_BATCH_BYTES", "default"),
               by_shape={})
    calls = args.warmup + args.reps
    for ns in shapes:
        wall = last_json(subprocess.run(child(args, ns), capture_output=True, text=True, timeout=args.timeout, cwd=ROOT),
                         f"N = {ns}: wall run")
        with tempfile.TemporaryDirectory() as d:
            r = subprocess.run(child(args, ns, ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"]),
                               capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
            last_json(r, f"N = {ns}: rocprofv3 run")
            traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            if len(traces) != 1:
                raise SystemExit(f"N = {ns}: expected one kernel trace, found {traces}")
            k = kernel_ms(traces[0], calls, args.warmup)
        ent = dict(wall_ms={kind: wall[kind]["median_ms"] for kind in wall}, wall_all_ms={kind: wall[kind]["all_ms"] for kind in wall},
                   kernels=k)
        ent["speedup_wall"] = wall["loop"]["median_ms"] / wall["grid"]["median_ms"]
        if "grid" in k:
            ent["speedup_kernel"] = k["loop"]["kernel_ms"] / k["grid"]["kernel_ms"]
        rec["by_shape"]["N=" + ns] = ent
        print(json.dumps({ns: ent}), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
