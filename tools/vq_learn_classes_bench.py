"""Measures class-batched codebook training against a loop of single-class trainings on one GPU; prints
one JSON record (optionally also written to --out).

Workload: K = 20 classes of corpus-shaped frames (e2vq_synth_frames_kind kind 1, one seed per class), class sizes spread
evenly over 2 000 .. 40 000 vectors in a seeded random order, P = 36, eps = 0.05, each class one .prd file.  For each
max M (default 1024, 2048):
  batched  e2vq_vq_learn_classes over the 20 files (vq learn --all-classes)
  loop     ecoz2_vq_learn once per class, one class after the other, in the same warm process
Both write their codebooks and reports (ECOZ2_VQ_QUIET=1, separate out roots); every timed pair is checked byte for byte.
The same on arrays, without files: e2vq_vq_train_classes (arrays_batched) against one VqSession ladder per class
(arrays_loop), the codebooks compared bit for bit.
Wall times: --warmup + --reps calls of each, the median of the timed calls.  Solo sweep: the batched call with
ECOZ2_VQ_LEARN_CLASSES_SOLO_FRAMES at each value of --solo (the classes above it train through the session path).
Cold CLI: one `ecoz2 vq learn --all-classes` process against 20 `ecoz2 vq learn --class-name` processes, each a fresh
child (trees compared).  Kernel times: a `rocprofv3 --kernel-trace --stats` run of its own per kind (batched, loop), one
call each, every kernel of the call summed.  --lo / --hi change the range of class sizes (the solo-threshold sweep of
DESIGN.md 4.9.1 also runs on 16 000 .. 320 000).
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLI = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
P, EPS = 36, 0.05
# the one-off kernels of a training set (re-layout, data statistics, the first codeword)
PROLOGUE = ("k_blockify", "k_global_sums", "k_finish_scalars", "k_finish_q", "k_init_codebook", "k_maxabs")


def make_corpus(d, K=20, lo=2000, hi=40000, seed=2026):
    import numpy as np

    import ecoz2rs_amd as e

    rng = np.random.default_rng(seed)
    sizes = [int(x) for x in rng.permutation(np.linspace(lo, hi, K).round().astype(int))]
    files = []
    for k, T in enumerate(sizes):
        name = f"c{k:02d}"
        p = os.path.join(d, "data", "predictors", name, "00000.prd")
        os.makedirs(os.path.dirname(p), exist_ok=True)
        e.formats.write_prd(p, name, e.synth.synth_frames_kind(seed + k, 1, 4, 0.05, P, 0, T))
        files.append(p)
    return sizes, files


def tree(d):
    out = {}
    for base, _dirs, names in os.walk(d):
        for n in names:
            p = os.path.join(base, n)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


def calls_of(files, work):
    import numpy as np

    import ecoz2rs_amd as e
    from ecoz2rs_amd import vq

    def batched(root):
        os.environ["ECOZ2_VQ_OUT_ROOT"] = root
        vq.vq_learn_classes(P, EPS, files)

    def loop(root):
        os.environ["ECOZ2_VQ_OUT_ROOT"] = root
        cb = e._lib.LEARN_CALLBACK(lambda *_a: None)
        for f in files:
            name = os.path.basename(os.path.dirname(f))
            fs, _keep = vq._to_vec_of_ptr_const_c_char([f])
            e.check(e.lib.ecoz2_vq_learn(P, EPS, name.encode(), fs, 1, None, cb))

    frames = [e.formats.read_prd(f)[2] for f in files]
    max_m = int(os.environ["ECOZ2_VQ_MAX_CODEBOOK_SIZE"])
    got = {}

    def arrays_batched():
        got["batched"] = [cb for cb, _lv in vq.train_codebooks(frames, P, EPS, max_m)]

    def arrays_loop():
        out = []
        for f in frames:
            with e.VqSession(P, device=0) as s:
                s.set_frames(f)
                s.prepare()
                s.init_codebook()
                s.learn(EPS, max_m)
                out.append(s.get_codebook())
        got["loop"] = out

    def arrays_same():
        return all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(got["batched"], got["loop"]))

    return dict(batched=lambda: batched(os.path.join(work, "b")), loop=lambda: loop(os.path.join(work, "l")),
                arrays_batched=arrays_batched, arrays_loop=arrays_loop), arrays_same


def run(args):
    """the measured calls of one max M (plain, or under rocprofv3 with --only); prints JSON"""
    os.environ["ECOZ2_VQ_QUIET"] = "1"
    os.environ["ECOZ2_VQ_MAX_CODEBOOK_SIZE"] = str(args.max_m)
    files = sorted(glob.glob(os.path.join(args.corpus, "data", "predictors", "*", "*.prd")))
    work = tempfile.mkdtemp()
    calls, arrays_same = calls_of(files, work)
    kinds = [args.only] if args.only else ["batched", "loop", "arrays_batched", "arrays_loop"]
    res = {}
    ts = {k: [] for k in kinds}
    for i in range(args.warmup + args.reps):
        for k in kinds:
            t0 = time.perf_counter()
            calls[k]()
            ts[k].append(time.perf_counter() - t0)
        if not args.only and tree(os.path.join(work, "b")) != tree(os.path.join(work, "l")):
            raise SystemExit("batched and loop outputs differ")
        if not args.only and not arrays_same():
            raise SystemExit("batched and loop codebooks differ")
    for k in kinds:
        res[k] = dict(median_ms=statistics.median(ts[k][args.warmup:]) * 1e3, all_ms=[round(x * 1e3, 2) for x in ts[k]])
    if args.solo and not args.only:
        sweep = {}
        for s in [int(x) for x in args.solo.split(",")]:
            os.environ["ECOZ2_VQ_LEARN_CLASSES_SOLO_FRAMES"] = str(s)
            t = []
            for _ in range(args.warmup + 3):
                t0 = time.perf_counter()
                calls["batched"]()
                t.append(time.perf_counter() - t0)
            if tree(os.path.join(work, "b")) != tree(os.path.join(work, "l")):
                raise SystemExit(f"solo threshold {s}: output differs")
            sweep[str(s)] = statistics.median(t[args.warmup:]) * 1e3
        del os.environ["ECOZ2_VQ_LEARN_CLASSES_SOLO_FRAMES"]
        res["solo_sweep_ms"] = sweep
    shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res))


def child(args, max_m, only=None, reps=None, warmup=None, extra=()):
    c = [*extra, sys.executable, os.path.abspath(__file__), "--run", "--corpus", args.corpus, "--max-m", str(max_m),
         "--reps", str(args.reps if reps is None else reps), "--warmup", str(args.warmup if warmup is None else warmup)]
    if only:
        c += ["--only", only]
    elif args.solo:
        c += ["--solo", args.solo]
    return c


def last_json(r, what):
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{what}: failed with status {r.returncode}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def kernel_ms(args, max_m, kind):
    """kernel time of one call, from a kernel trace of its own"""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(child(args, max_m, only=kind, reps=1, warmup=0,
                                 extra=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"]),
                           capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
        last_json(r, f"M = {max_m} {kind}: rocprofv3 run")
        traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if len(traces) != 1:
            raise SystemExit(f"expected one kernel trace, found {traces}")
        rows = sorted((int(x["Start_Timestamp"]), int(x["End_Timestamp"]), x["Kernel_Name"]) for x in csv.DictReader(open(traces[0])))
    by = {}
    for a, b, n in rows:
        n = n.split("(")[0].replace("void ", "")
        by[n] = by.get(n, 0.0) + (b - a) / 1e6
    top = sorted(by.items(), key=lambda kv: -kv[1])[:8]
    prologue = sum(v for k, v in by.items() if any(p in k for p in PROLOGUE))
    return dict(kernel_ms=sum(by.values()), prologue_kernel_ms=prologue, launches=len(rows), span_ms=(rows[-1][1] - rows[0][0]) / 1e6 if rows else 0,
                top_kernels_ms={k: round(v, 3) for k, v in top})


def cold_cli(args, max_m, sizes):
    env = dict(os.environ, ECOZ2_VQ_QUIET="1", ECOZ2_VQ_MAX_CODEBOOK_SIZE=str(max_m))
    for k in ("ECOZ2_VQ_LEARN_CLASSES_SOLO_FRAMES", "ECOZ2_VQ_LEARN_BATCH_BYTES", "ECOZ2_VQ_GPUS"):
        env.pop(k, None)
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        r = subprocess.run([CLI, "vq", "learn", "--all-classes", "-P", str(P), "--predictors", "data/predictors"], cwd=args.corpus,
                           env=dict(env, ECOZ2_VQ_OUT_ROOT=os.path.join(d, "b")), capture_output=True, text=True,
                           timeout=args.timeout)
        t_b = time.perf_counter() - t0
        if r.returncode != 0 or "classes: 20" not in r.stdout:
            raise SystemExit("cold --all-classes failed: " + r.stdout[-2000:] + r.stderr[-2000:])
        t0 = time.perf_counter()
        for k in range(len(sizes)):
            name = f"c{k:02d}"
            r = subprocess.run([CLI, "vq", "learn", "-P", str(P), "--class-name", name, "--predictors", f"data/predictors/{name}"],
                               cwd=args.corpus, env=dict(env, ECOZ2_VQ_OUT_ROOT=os.path.join(d, "l")), capture_output=True,
                               text=True, timeout=args.timeout)
            if r.returncode != 0:
                raise SystemExit("cold single-class run failed: " + r.stderr[-2000:])
        t_l = time.perf_counter() - t0
        same = tree(os.path.join(d, "b")) == tree(os.path.join(d, "l"))
    if not same:
        raise SystemExit("cold CLI outputs differ")
    return dict(all_classes_s=t_b, loop_20_processes_s=t_l, speedup=t_l / t_b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true", help="(internal) the measured calls")
    ap.add_argument("--corpus")
    ap.add_argument("--max-m", type=int, default=1024)
    ap.add_argument("--max-ms", default="1024,2048")
    ap.add_argument("--only")
    ap.add_argument("--solo", default="0,4000,8000,16000,24000,32000,524288")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-cold", action="store_true")
    ap.add_argument("--lo", type=int, default=2000, help="smallest class")
    ap.add_argument("--hi", type=int, default=40000, help="largest class")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child run")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.run:
        return run(args)
    with tempfile.TemporaryDirectory() as corpus:
        args.corpus = corpus
        sizes, _files = make_corpus(corpus, lo=args.lo, hi=args.hi)
        rec = dict(tool="tools/vq_learn_classes_bench.py", argv=sys.argv[1:], K=len(sizes), P=P, eps=EPS, sizes=sizes, total_frames=sum(sizes),
                   reps=args.reps, warmup=args.warmup, by_max_M={})
        for max_m in [int(x) for x in args.max_ms.split(",")]:
            solo = args.solo if max_m == int(args.max_ms.split(",")[0]) else ""
            a2 = argparse.Namespace(**{**vars(args), "solo": solo})
            wall = last_json(subprocess.run(child(a2, max_m), capture_output=True, text=True, timeout=args.timeout, cwd=ROOT),
                             f"M = {max_m}: wall run")
            kinds = ("batched", "loop", "arrays_batched", "arrays_loop")
            ent = dict(wall_ms={k: wall[k]["median_ms"] for k in kinds}, wall_all_ms={k: wall[k]["all_ms"] for k in kinds})
            ent["speedup_wall"] = wall["loop"]["median_ms"] / wall["batched"]["median_ms"]
            ent["speedup_wall_arrays"] = wall["arrays_loop"]["median_ms"] / wall["arrays_batched"]["median_ms"]
            if "solo_sweep_ms" in wall:
                ent["solo_sweep_ms"] = wall["solo_sweep_ms"]
            if not args.no_trace:
                ent["kernels"] = {k: kernel_ms(a2, max_m, k) for k in ("batched", "loop")}
                ent["speedup_kernel"] = ent["kernels"]["loop"]["kernel_ms"] / ent["kernels"]["batched"]["kernel_ms"]
            if not args.no_cold:
                ent["cold_cli"] = cold_cli(args, max_m, sizes)
            rec["by_max_M"][str(max_m)] = ent
            print(json.dumps({max_m: ent}), file=sys.stderr)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
