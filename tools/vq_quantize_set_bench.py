"""Measures `vq quantize --codebooks` (one pass over a set of codebooks) against the loop of single-codebook
calls on one GPU; prints one JSON record and writes it to --out (default profiles/vq_quantize_set_bench.json).

A ladder of codebooks M = 2 .. 2048, P = 36, is trained once with `vq learn` on 2^18 corpus-shaped frames
(e2vq_synth_frames_kind, kind 1).  Workloads, each in a child process of its own under a timeout (the tool stops at the
first failing step), set call and loop alternating in the same warm process after --warmup rounds of both, the median of
--reps timed rounds and the spread (max - min) of each side, every timed pair compared byte for byte:
  files_short  e2vq_vq_quantize_codebooks over 5 000 .prd of 400 frames against ecoz2_vq_quantize once per codebook
  files_long   the same over 8 .prd of 1.25 M frames (page cache warm)
  resident     e2vq_cbset_quantize_device against K sessions x e2vq_quantize_device on 2^21 frames on the device, wall time
               ending in a synchronise
Kernel time: a `rocprofv3 --kernel-trace --stats` run of its own per side of the resident workload, every kernel of one call
summed; the loop's sessions are synchronised one after the other there, so that no kernel's duration is stretched by a
neighbour on another stream (in the wall-time rounds they overlap, as a caller's would).  Frames fetched: a counter run of
its own (`--pmc FETCH_SIZE`, no tracing) for k_quantize_set; the counter reports half the bytes of a wide coalesced read
on gfx950, the record holds both the counter's figure and the doubled one.
--short-files / --short-frames / --long-files / --long-frames / --resident-frames scale the workloads.
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
P, EPS, SEED = 36, 0.05, 2027
MS = [2 << i for i in range(11)]


def tree(d):
    out = {}
    for base, _dirs, names in os.walk(d):
        for n in names:
            p = os.path.join(base, n)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


def codebook_files(work):
    return [os.path.join(work, "data", "codebooks", "_", f"eps_{EPS:g}_M_{M:04d}.cbook") for M in MS]


def prepare(args):
    """the ladder and the two corpora (GPU: the ladder's training)"""
    import ecoz2rs_amd as e
    from ecoz2rs_amd import vq

    os.environ.update(ECOZ2_VQ_QUIET="1", ECOZ2_VQ_OUT_ROOT=args.work, ECOZ2_VQ_MAX_CODEBOOK_SIZE=str(MS[-1]))
    train = os.path.join(args.work, "train.prd")
    e.formats.write_prd(train, "_", e.synth.synth_frames_kind(SEED, 1, 4, 0.05, P, 0, 1 << 18))
    vq.vq_learn(None, P, EPS, "_", [train])
    assert all(os.path.exists(f) for f in codebook_files(args.work))
    for name, n, T in (("short", args.short_files, args.short_frames), ("long", args.long_files, args.long_frames)):
        for i in range(n):
            p = os.path.join(args.work, name, f"c{i % 8}", f"{i:05d}.prd")
            os.makedirs(os.path.dirname(p), exist_ok=True)
            e.formats.write_prd(p, f"c{i % 8}", e.synth.synth_frames_kind(SEED + 1, 1, 4, 0.05, P, (1 << 18) + i * T, T))
    print(json.dumps(dict(prepared=True)))


def timed_rounds(args, set_call, loop_call, same):
    ts = dict(set=[], loop=[])
    for i in range(args.warmup + args.reps):
        for k, fn in (("set", set_call), ("loop", loop_call)) if i % 2 == 0 else (("loop", loop_call), ("set", set_call)):
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
        if not same():
            raise SystemExit("set call and loop differ")
    out = {}
    for k in ts:
        t = [x * 1e3 for x in ts[k][args.warmup:]]
        out[k] = dict(median_ms=statistics.median(t), spread_ms=max(t) - min(t), all_ms=[round(x * 1e3, 2) for x in ts[k]])
    out["speedup"] = out["loop"]["median_ms"] / out["set"]["median_ms"]
    out["gain_ms"] = out["loop"]["median_ms"] - out["set"]["median_ms"]
    out["faster_beyond_spread"] = out["gain_ms"] > max(out["set"]["spread_ms"], out["loop"]["spread_ms"])
    return out


def run_files(args, name):
    import ecoz2rs_amd as e
    from ecoz2rs_amd import vq

    os.environ["ECOZ2_VQ_QUIET"] = "1"
    files = sorted(glob.glob(os.path.join(args.work, name, "*", "*.prd")))
    cbs = codebook_files(args.work)
    fs, _keep = vq._to_vec_of_ptr_const_c_char(files)
    cs, _keep2 = vq._to_vec_of_ptr_const_c_char(cbs)
    roots = {k: os.path.join(args.work, f"out_{name}_{k}") for k in ("set", "loop")}
    devnull = os.open(os.devnull, os.O_WRONLY)
    stdout = os.dup(1)

    def quiet(fn):
        sys.stdout.flush()
        os.dup2(devnull, 1)
        try:
            fn()
        finally:
            os.dup2(stdout, 1)

    def set_call():
        os.environ["ECOZ2_VQ_OUT_ROOT"] = roots["set"]
        quiet(lambda: e.check(e.lib.e2vq_vq_quantize_codebooks(cs, len(cbs), fs, len(files), 0)))

    def loop_call():
        os.environ["ECOZ2_VQ_OUT_ROOT"] = roots["loop"]
        for cb in cbs:
            quiet(lambda: e.check(e.lib.ecoz2_vq_quantize(cb.encode(), fs, len(files), 0)))

    res = timed_rounds(args, set_call, loop_call, lambda: tree(roots["set"]) == tree(roots["loop"]))
    res.update(files=len(files), frames=sum(e.formats.read_prd(f)[2].shape[0] for f in files[:1]) * len(files), codebooks=len(cbs))
    for r in roots.values():
        shutil.rmtree(r, ignore_errors=True)
    print(json.dumps(res))


def run_resident(args):
    import torch

    torch.cuda.init()  # (before the library: torch brings its own copy of the HIP runtime)
    import ecoz2rs_amd as e

    T, K = args.resident_frames, len(MS)
    cbs = [e.formats.read_cbook(f)[-1] for f in codebook_files(args.work)]
    frames = torch.from_numpy(e.synth.synth_frames_kind(SEED + 2, 1, 4, 0.05, P, 1 << 22, T)).to("cuda:0")
    sym = [torch.zeros((K, T), dtype=torch.int16, device="cuda:0") for _ in range(2)]
    dmin = [torch.zeros((K, T), dtype=torch.float64, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    cset = e.CodebookSet(P, cbs)
    sessions = [e.VqSession(P) for _ in cbs]
    for s, cb in zip(sessions, cbs):
        s.set_codebook(cb)

    def set_call():
        cset.quantize_device(frames, T, sym[0], T, dmin[0], T)
        cset.set_stream(None)  # (synchronises the set's stream)

    def loop_call():
        for k, s in enumerate(sessions):
            s.quantize_device(frames, T, sym[1][k], dmin[1][k])
        for s in sessions:
            s.synchronize()

    kinds = dict(set=set_call, loop=loop_call)
    def loop_serial():  # (one session after the other: kernel durations that no concurrent stream inflates)
        for k, s in enumerate(sessions):
            s.quantize_device(frames, T, sym[1][k], dmin[1][k])
            s.synchronize()

    if args.only:  # (under the profiler: one warm-up call, one more; the loop's sessions serialised)
        kinds["loop"] = loop_serial
        kinds[args.only]()
        kinds[args.only]()
        print(json.dumps(dict(only=args.only, set_launches=cset.launch_counts()[0])))
        return
    res = timed_rounds(args, set_call, loop_call, lambda: torch.equal(sym[0], sym[1]) and torch.equal(dmin[0].view(torch.int64), dmin[1].view(torch.int64)))
    res.update(frames=T, codebooks=K, launch_counts_per_call=[x // (args.warmup + args.reps) for x in cset.launch_counts()])
    print(json.dumps(res))


def child(args, what, only=None, extra=()):
    c = [*extra, sys.executable, os.path.abspath(__file__), "--step", what, "--work", args.work, "--reps", str(args.reps), "--warmup",
         str(args.warmup)]
    for k in ("short_files", "short_frames", "long_files", "long_frames", "resident_frames"):
        c += ["--" + k.replace("_", "-"), str(getattr(args, k))]
    return c + (["--only", only] if only else [])


def step(args, what, only=None, extra=(), want_json=True):
    """one GPU step under its own timeout; the tool stops at the first one that fails"""
    r = subprocess.run(["timeout", "-k", "10", str(args.timeout), *child(args, what, only, extra)], capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{what}{' ' + only if only else ''}: failed with status {r.returncode}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]) if want_json else r


def kernel_ms(args, side):
    with tempfile.TemporaryDirectory() as d:
        step(args, "resident", only=side, extra=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"])
        traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if len(traces) != 1:
            raise SystemExit(f"expected one kernel trace, found {traces}")
        rows = sorted((int(x["Start_Timestamp"]), int(x["End_Timestamp"]), x["Kernel_Name"]) for x in csv.DictReader(open(traces[0])))
    by, n = {}, {}
    for a, b, name in rows:
        name = name.split("(")[0].replace("void ", "")
        by[name] = by.get(name, 0.0) + (b - a) / 1e6
        n[name] = n.get(name, 0) + 1
    # two calls ran (one warm-up): a call is half of every sweep kernel's time; the image kernels of the first call stay whole
    sweeps = {k: v / 2 for k, v in by.items() if any(s in k for s in ("k_quantize_set", "k_pass_mfma", "k_pass_pre"))}
    return dict(kernel_ms_per_call=sum(sweeps.values()), per_call_ms={k: round(v, 4) for k, v in sorted(sweeps.items(), key=lambda kv: -kv[1])},
                launches_two_calls={k: n[k] for k in sweeps})


def fetch_size(args):
    with tempfile.TemporaryDirectory() as d:
        step(args, "resident", only="set", extra=["rocprofv3", "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", d, "--"])
        files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
        if len(files) != 1:
            raise SystemExit(f"expected one counter file, found {files}")
        vals = [float(x["Counter_Value"]) for x in csv.DictReader(open(files[0]))
                if "k_quantize_set" in x["Kernel_Name"] and x["Counter_Name"] == "FETCH_SIZE"]
    if not vals:
        raise SystemExit("no FETCH_SIZE sample of k_quantize_set")
    kb = vals[-1]  # (the counter is in kilobytes; the last launch: the warm one)
    # gfx950 tallies the 128-byte requests of a wide coalesced read at 64 bytes: FETCH_SIZE is half the bytes read
    return dict(fetch_kbytes=kb, counter_bytes_per_frame=kb * 1024 / args.resident_frames,
                bytes_per_frame=2 * kb * 1024 / args.resident_frames, payload_bytes_per_frame=(P + 1) * 8,
                note="bytes_per_frame = 2 x FETCH_SIZE: the counter reports half of a 16-B-per-lane streaming read on gfx950")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", help="(internal) prepare | files_short | files_long | resident")
    ap.add_argument("--work")
    ap.add_argument("--only")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--short-files", type=int, default=5000)
    ap.add_argument("--short-frames", type=int, default=400)
    ap.add_argument("--long-files", type=int, default=8)
    ap.add_argument("--long-frames", type=int, default=1250000)
    ap.add_argument("--resident-frames", type=int, default=1 << 21)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--timeout", type=int, default=420, help="seconds per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vq_quantize_set_bench.json"))
    args = ap.parse_args()
    if args.step:
        return dict(prepare=lambda: prepare(args), files_short=lambda: run_files(args, "short"), files_long=lambda: run_files(args, "long"),
                    resident=lambda: run_resident(args))[args.step]()
    if args.reps < 5:
        raise SystemExit("at least 5 timed repetitions")
    with tempfile.TemporaryDirectory() as work:
        args.work = work
        rec = dict(tool="tools/vq_quantize_set_bench.py", argv=sys.argv[1:], P=P, eps=EPS, Ms=MS, reps=args.reps, warmup=args.warmup)
        step(args, "prepare")
        for what in ("files_short", "files_long", "resident"):
            rec[what] = step(args, what)
            print(json.dumps({what: rec[what]}), file=sys.stderr)
        if not args.no_trace:
            rec["kernel_time"] = {side: kernel_ms(args, side) for side in ("set", "loop")}
            rec["kernel_time"]["speedup"] = rec["kernel_time"]["loop"]["kernel_ms_per_call"] / rec["kernel_time"]["set"]["kernel_ms_per_call"]
            rec["frames_fetched"] = fetch_size(args)
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
