"""Measures the E-step of `hmm learn --loop` next to the passes it is built from, on the same models and
stream in the same session; prints one JSON record (optionally also written to --out).

The workload is tools/hmm_trans_posteriors_bench.py's: one stream of --t random symbols (default 38 265), M = 1024, K = 20
random models of N states each, the planted matrix of 4.8.8 plus --ln-switch (default -5).  Per N (default 5, 16, 32):
  loop_estep        one e2vq_hmm_loop_estep call without acc_trans: k_hmm_loop_estep<.., false>
  loop_estep_gram   the same with acc_trans: k_hmm_loop_estep<.., true>
  trans_estep       one e2vq_hmm_transitions_estep call: k_hmm_trans_estep -- the forward-backward pass and the bigram counts
                    alone (`over_trans_estep`)
  embed_fb          one e2vq_hmm_embedded_estep call on the same stream with the 20 classes as its transcript, each once:
                    k_hmm_embed_fb -- the state counts of a chain of 20 units (`over_embed_fb`)
The comparators are code this feature does not touch; the commit before it cannot compute these counts, so no speed-up is
claimed.  --warmup + --reps of each.  Kernel times come from one `rocprofv3 --kernel-trace` run of this script (--run) per N,
without counters; each call's own HIP-event time is recorded next to it.  median and min .. max over the repetitions.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hmm_trans_posteriors_bench import workload  # noqa: E402

KINDS = {
    "loop_estep": re.compile(r"k_hmm_loop_estep<\w+, \w+, false>"),
    "loop_estep_gram": re.compile(r"k_hmm_loop_estep<\w+, \w+, true>"),
    "trans_estep": re.compile(r"k_hmm_trans_estep"),
    "embed_fb": re.compile(r"k_hmm_embed_fb"),
}


def run(args):
    """the measured calls (under rocprofv3); prints wall and HIP-event times as JSON"""
    import numpy as np

    import ecoz2rs_amd as e

    models, sym, lt = workload(args.n, args.m, args.k, args.t, args.ln_switch)
    offs = np.array([0, len(sym)], dtype=np.int64)
    units, unit_offs = np.arange(args.k, dtype=np.int32), np.array([0, args.k], dtype=np.int64)
    out = {}
    calls = (("loop_estep", lambda: e.hmm.loop_estep(models, sym, offs, lt), e.hmm.loop_estep_last_kernel_ms),
             ("loop_estep_gram", lambda: e.hmm.loop_estep(models, sym, offs, lt, acc_trans=True), e.hmm.loop_estep_last_kernel_ms),
             ("trans_estep", lambda: e.hmm.transitions_estep(models, sym, offs, lt), e.hmm.transitions_estep_last_kernel_ms),
             ("embed_fb", lambda: e.hmm.embedded_estep(models, sym, offs, units, unit_offs, ln_switch=args.ln_switch),
              e.hmm.embedded_last_kernel_ms))
    for kind, call, event in calls:
        ts, ev = [], []
        for _ in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            r = call()
            ts.append((time.perf_counter() - t0) * 1e3)
            ev.append(event())
        out[kind] = dict(call_wall_ms=statistics.median(ts[args.warmup:]), event_ms=statistics.median(ev[args.warmup:]),
                         event_ms_min=min(ev[args.warmup:]), event_ms_max=max(ev[args.warmup:]), status=r["status"].tolist())
    print(json.dumps(out))


def kernel_ms(trace, calls, warmup):
    """per kind the kernel time of each call"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true", help="(internal) the measured calls, for rocprofv3")
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--ns", default="5,16,32")
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--t", type=int, default=38265)
    ap.add_argument("--ln-switch", type=float, default=-5.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.run:
        return run(args)
    rec = dict(tool="tools/hmm_loop_em_bench.py", M=args.m, K=args.k, T=args.t, ln_switch=args.ln_switch, reps=args.reps,
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
            if all("kernel_ms" in k[kind] for kind in KINDS):
                ent["over_trans_estep"] = k["loop_estep"]["kernel_ms"] / k["trans_estep"]["kernel_ms"]
                ent["gram_over_trans_estep"] = k["loop_estep_gram"]["kernel_ms"] / k["trans_estep"]["kernel_ms"]
                ent["gram_over_plain"] = k["loop_estep_gram"]["kernel_ms"] / k["loop_estep"]["kernel_ms"]
                ent["over_embed_fb"] = k["loop_estep"]["kernel_ms"] / k["embed_fb"]["kernel_ms"]
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
