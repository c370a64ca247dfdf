"""Measures grid-batched HMM scoring against a loop of single scorings on one GPU; prints one JSON
record (optionally also written to --out).

Workload: K = 20 class models (e2vq_hmm_init type 3) per (N, M) and S = 1 000 test sequences of T = 300 symbols per
codebook size M (drawn around class-specific ramps), over the grid N in --ns x M in --ms (default {5, 16, 32, 64} x
{64, 128, 256, 512, 1024}).  Shapes: each N alone over all M, and the whole grid.  Per shape, alternating within one warm
process:
  grid      one e2vq_hmm_score_grid call over every model of the shape (k_hmm_score_grid at the widths in use: floor(64 / N)
            models a wave for N <= 21, one above)
  packed    the same call with ECOZ2_HMM_SCORE_PACK=1 (floor(64 / N) models a wave for every N <= 32)
  unpacked  the same call with ECOZ2_HMM_SCORE_PACK=0 (one model a wave at every N)
  loop      e2vq_hmm_score once per (N, M) of the shape, one after the other (k_hmm_score: the path before the grid call)
  loop_b    the loop again: |loop - loop_b| / loop is the spread of the loop against itself
Wall times: --warmup + --reps rounds of the four in a plain run (no tracer), each call ending in its own synchronise, the
median of the timed calls (the Python wrappers' packing of the arrays included, in every arm).  Kernel times: a `rocprofv3 --kernel-trace` run of its own (the same calls), the launches cut
into calls by their count per round, the warm-up rounds dropped, the median over the rounds reported.  `speedup` is
loop / grid.  --files adds the file-level comparison on a smaller corpus: one `ecoz2 hmm classify --grid` process against
one `ecoz2 hmm classify` process per (N, M).
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
KINDS = ("grid", "packed", "unpacked", "loop", "loop_b")


def workload(Ns, Ms, K, S, T, seed=2026):
    """-> models [(pi, A, B)] in grid order, the shared sequences, each model's range"""
    import numpy as np

    import ecoz2rs_amd as e

    rng = np.random.default_rng(seed)
    seqs, m_range = [], {}
    for M in Ms:
        ramp = np.linspace(0, M - 1, T)
        lo = len(seqs)
        seqs += [np.clip((ramp * (0.5 + (q % K) / (2 * K)) + rng.normal(0, M / 16, T)).round(), 0, M - 1).astype(np.uint16)
                 for q in range(S)]
        m_range[M] = (lo, len(seqs))
    models, ranges = [], []
    for N in Ns:
        for M in Ms:
            e.hmm.set_random_seed(seed + N + M)
            for _k in range(K):
                models.append(e.hmm.init_model(N, M, 3))
                ranges.append(m_range[M])
    return models, seqs, ranges


def calls_of(args):
    import ecoz2rs_amd as e

    Ns, Ms = [int(x) for x in args.ns.split(",")], [int(x) for x in args.ms.split(",")]
    models, seqs, ranges = workload(Ns, Ms, args.k, args.s, args.t)
    per_point = [(models[i:i + args.k], seqs[ranges[i][0]:ranges[i][1]]) for i in range(0, len(models), args.k)]

    def grid(pack):
        os.environ.pop("ECOZ2_HMM_SCORE_PACK", None)
        if pack is not None:
            os.environ["ECOZ2_HMM_SCORE_PACK"] = pack
        try:
            return e.hmm.score_grid(models, seqs, ranges)
        finally:
            os.environ.pop("ECOZ2_HMM_SCORE_PACK", None)

    loop = lambda: [e.hmm.score(ms, ss) for ms, ss in per_point]
    return {"grid": lambda: grid(None), "packed": lambda: grid("1"), "unpacked": lambda: grid("0"), "loop": loop, "loop_b": loop}


def run(args):
    """the measured calls (plain, or under rocprofv3); prints the wall times as JSON"""
    fns = calls_of(args)
    ts = {k: [] for k in KINDS}
    for _ in range(args.warmup + args.reps):
        for kind in KINDS:  # (the arms alternate within the run)
            t0 = time.perf_counter()
            fns[kind]()
            ts[kind].append(time.perf_counter() - t0)
    print(json.dumps({k: dict(median_ms=statistics.median(v[args.warmup:]) * 1e3, all_ms=[round(x * 1e3, 3) for x in v])
                      for k, v in ts.items()}))


def kernel_ms(trace, rounds, warmup):
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0]) for r in csv.DictReader(open(trace))
                  if "k_hmm_score" in r["Kernel_Name"])
    out = {}
    packed = [r for r in rows if "k_hmm_score_grid" in r[2]]
    single = [r for r in rows if "k_hmm_score_grid" not in r[2] and "k_hmm_score_wg" not in r[2]]
    if len(packed) + len(single) != len(rows) or not packed or not single or len(packed) % (3 * rounds) or len(single) % (2 * rounds):
        return dict(error=f"{len(packed)} grid and {len(single)} single launches of {len(rows)} in {rounds} rounds")
    for kinds, sel in ((("grid", "packed", "unpacked"), packed), (("loop", "loop_b"), single)):
        n, per = len(kinds), len(sel) // (len(kinds) * rounds)
        for h, kind in enumerate(kinds):
            sums = [sum(b - a for a, b, _ in sel[(n * c + h) * per:(n * c + h + 1) * per]) / 1e6 for c in range(rounds)]
            out[kind] = dict(kernel_ms=statistics.median(sums[warmup:]), launches_per_call=per)
    return out


def child(args, ns, extra=()):
    return [*extra, sys.executable, os.path.abspath(__file__), "--run", "--ns", ns, "--ms", args.ms, "--k", str(args.k),
            "--s", str(args.s), "--t", str(args.t), "--reps", str(args.reps), "--warmup", str(args.warmup)]


def last_json(r, what):
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{what}: failed with status {r.returncode}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def files_comparison(args):
    """one `ecoz2 hmm classify --grid` process against one `ecoz2 hmm classify` process per (N, M), on files"""
    import ecoz2rs_amd as e

    exe = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
    Ns, Ms = [int(x) for x in args.ns.split(",")], [int(x) for x in args.ms.split(",")]
    models, seqs, ranges = workload(Ns, Ms, args.k, args.file_s, args.t)
    with tempfile.TemporaryDirectory() as d:
        i = 0
        for N in Ns:
            for M in Ms:
                os.makedirs(f"{d}/hmms/N{N}__M{M}")
                for k in range(args.k):
                    e.hmm.save_model(f"{d}/hmms/N{N}__M{M}/C{k:02d}.hmm", f"C{k:02d}", *models[i])
                    i += 1
        for M in Ms:
            lo, hi = ranges[Ms.index(M) * args.k]
            for q in range(lo, hi):
                p = f"{d}/seqs/M{M}/C{(q - lo) % args.k:02d}"
                os.makedirs(p, exist_ok=True)
                e.formats.write_seq(f"{p}/{q - lo:05d}.seq", f"C{(q - lo) % args.k:02d}", M, seqs[q])
        quiet = dict(stdout=subprocess.DEVNULL, check=True, cwd=d, timeout=args.timeout)
        grid = [exe, "hmm", "classify", "--grid", "--models", "hmms", "--tt", "TEST", "--sequences", "seqs"]
        loop = [[exe, "hmm", "classify", "--models", f"hmms/N{N}__M{M}", "--tt", "TEST", "-M", str(M), "--sequences", f"seqs/M{M}"]
                for N in Ns for M in Ms]
        ts = {"grid": [], "loop": []}
        for _ in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            subprocess.run(grid, **quiet)
            ts["grid"].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for cmd in loop:
                subprocess.run(cmd, **quiet)
            ts["loop"].append(time.perf_counter() - t0)
    out = {k: dict(median_ms=statistics.median(v[args.warmup:]) * 1e3, all_ms=[round(x * 1e3, 1) for x in v]) for k, v in ts.items()}
    out.update(sequences_per_M=args.file_s, processes_in_loop=len(loop), speedup=out["loop"]["median_ms"] / out["grid"]["median_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true", help="(internal) the measured calls")
    ap.add_argument("--ns", default="5,16,32,64")
    ap.add_argument("--ms", default="64,128,256,512,1024")
    ap.add_argument("--shapes", default=None, help="';'-separated N lists (default: each N alone, then all of --ns)")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--s", type=int, default=1000, help="test sequences per M")
    ap.add_argument("--t", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child run")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 runs (wall times only)")
    ap.add_argument("--files", action="store_true", help="also the file-level comparison (processes)")
    ap.add_argument("--file-s", type=int, default=200, help="test sequences per M of the file-level comparison")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.run:
        return run(args)
    shapes = args.shapes.split(";") if args.shapes else args.ns.split(",") + [args.ns]
    rec = dict(tool="tools/hmm_classify_grid_bench.py", K=args.k, S_per_M=args.s, T=args.t, Ms=args.ms, reps=args.reps,
               warmup=args.warmup, by_shape={})
    rounds = args.warmup + args.reps
    for ns in shapes:
        wall = last_json(subprocess.run(child(args, ns), capture_output=True, text=True, timeout=args.timeout, cwd=ROOT),
                         f"N = {ns}: wall run")
        ent = dict(wall_ms={kind: wall[kind]["median_ms"] for kind in wall}, wall_all_ms={kind: wall[kind]["all_ms"] for kind in wall})
        ent["speedup_wall"] = wall["loop"]["median_ms"] / wall["grid"]["median_ms"]
        ent["loop_spread_wall"] = abs(wall["loop"]["median_ms"] - wall["loop_b"]["median_ms"]) / wall["loop"]["median_ms"]
        if not args.no_trace:
            with tempfile.TemporaryDirectory() as d:
                r = subprocess.run(child(args, ns, ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"]),
                                   capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
                last_json(r, f"N = {ns}: rocprofv3 run")
                traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
                if len(traces) != 1:
                    raise SystemExit(f"N = {ns}: expected one kernel trace, found {traces}")
                k = kernel_ms(traces[0], rounds, args.warmup)
            ent["kernels"] = k
            if "grid" in k:
                ent["speedup_kernel"] = k["loop"]["kernel_ms"] / k["grid"]["kernel_ms"]
                ent["loop_spread_kernel"] = abs(k["loop"]["kernel_ms"] - k["loop_b"]["kernel_ms"]) / k["loop"]["kernel_ms"]
        rec["by_shape"]["N=" + ns] = ent
        print(json.dumps({ns: ent}), file=sys.stderr, flush=True)
    if args.files:
        rec["files"] = files_comparison(args)
        print(json.dumps({"files": rec["files"]}), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
