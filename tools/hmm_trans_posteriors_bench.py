"""Measures `hmm segment --class-transitions --grammar-posteriors` next to its two siblings on the same
models and stream in the same session; prints one JSON record (optionally also written to --out).

One stream of --t random symbols (default 38 265), M = 1024, K = 20 random models (e2vq_hmm_init type 0) of N states each.
The prices are those of tools/hmm_segment_trans_bench.py: hmm.class_transitions (alpha = 1) of its planted label sequence
plus --ln-switch (default -5).  Per N (default 5, 16, 32):
  trans_posteriors  one e2vq_hmm_segment_trans_posteriors call: k_hmm_loop_posteriors_trans
  posteriors        one e2vq_hmm_segment_posteriors call at ln_switch alone: k_hmm_loop_posteriors (resident) -- what the
                    matrix costs a posterior pass (`over_posteriors`)
  trans             one e2vq_hmm_segment_trans call: k_hmm_segment_trans + k_hmm_segment_trans_backtrack -- what a posterior
                    pass costs a decode under the same matrix (`over_trans`)
The two comparators are code this feature does not touch; the commit before it cannot compute the quantity, so no speed-up
is claimed.  --warmup + --reps of each.  Kernel times come from one `rocprofv3 --kernel-trace` run of this script (--run)
per N, without counters; each call's own HIP-event time is recorded next to it.  median and min .. max over the repetitions.
--bodies (a list of auto, resident, looped: ECOZ2_HMM_TRANS_FB_BODY of the trans_posteriors calls): a run per N and body,
by_N[N][body], and looped_over_resident where both ran -- the price of the looped body where the resident one runs.  In such a
run the two comparators take their own bodies under auto, so that a packing of more than 16 wave-slots (N = 64 at K = 20) is
measured against k_hmm_loop_posteriors_looped and k_hmm_segment_trans_looped.  A packing the body refuses is recorded as
refused, with the library's message.  Without --bodies, one run per N with the environment's body, by_N[N], as before.
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
    "trans_posteriors": re.compile(r"k_hmm_loop_posteriors_trans"),
    "posteriors": re.compile(r"k_hmm_loop_posteriors(_looped)?(<|\b(?!_))"),
    "trans": re.compile(r"k_hmm_segment_trans"),
}


def workload(N, M, K, T, ln_switch, seed=2026):
    import numpy as np

    import ecoz2rs_amd as e

    e.hmm.set_random_seed(seed + N)
    models = [e.hmm.init_model(N, M, 0) for _ in range(K)]
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, M, T).astype(np.uint16)
    labels = [0]
    for _ in range(1999):
        labels.append((labels[-1] + 1) % K if rng.uniform() < 0.9 else int(rng.integers(0, K)))
    lt = e.hmm.class_transitions([labels], K, 1.0) + ln_switch
    return models, sym, lt


def run(args):
    """the measured calls (under rocprofv3); prints wall and HIP-event times as JSON"""
    import numpy as np

    import ecoz2rs_amd as e

    models, sym, lt = workload(args.n, args.m, args.k, args.t, args.ln_switch)
    offs = np.array([0, len(sym)], dtype=np.int64)
    out = {}

    def trans_posteriors(sym=sym, offs=offs):
        with e.hmm.trans_fb_body(args.body):
            return e.hmm.segment_trans_posteriors(models, sym, offs, lt)

    if args.body:
        try:
            trans_posteriors(sym[:8], [0, 8])
        except e.Ecoz2Error as err:
            print(json.dumps(dict(refused=str(err))))
            return
    others = "auto" if args.body else None  # (the comparators' own variables)
    calls = (("trans_posteriors", trans_posteriors, e.hmm.segment_trans_posteriors_last_kernel_ms),
             ("posteriors", lambda: e.hmm.segment_posteriors(models, sym, offs, args.ln_switch, body=others or "resident"),
              e.hmm.segment_posteriors_last_kernel_ms),
             ("trans", lambda: e.hmm.segment_trans(models, sym, offs, lt, body=others), e.hmm.segment_trans_last_kernel_ms))
    for kind, call, event in calls:
        ts, ev = [], []
        for _ in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
            ev.append(event())
        out[kind] = dict(call_wall_ms=statistics.median(ts[args.warmup:]), event_ms=statistics.median(ev[args.warmup:]),
                         event_ms_min=min(ev[args.warmup:]), event_ms_max=max(ev[args.warmup:]))
    print(json.dumps(out))


def kernel_ms(trace, calls, warmup, skip=None):
    """per kind the kernel time of each call; skip[kind]: launches before the measured calls (the probe of `run`)"""
    rows = list(csv.DictReader(open(trace)))
    out = {}
    for kind, rx in KINDS.items():
        sel = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows if rx.search(r["Kernel_Name"]))
        sel = sel[(skip or {}).get(kind, 0):]
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
    ap.add_argument("--body", help="(internal) the body of the run")
    ap.add_argument("--bodies", help="auto, resident and / or looped, comma-separated: a run per N and body")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.run:
        return run(args)
    rec = dict(tool="tools/hmm_trans_posteriors_bench.py", M=args.m, K=args.k, T=args.t, ln_switch=args.ln_switch, reps=args.reps,
               warmup=args.warmup, by_N={})
    bodies = args.bodies.split(",") if args.bodies else [None]
    if args.bodies:
        rec["bodies"] = bodies
    for N in [int(x) for x in args.ns.split(",")]:
        ents = {}
        for body in bodies:
            with tempfile.TemporaryDirectory() as d:
                cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--",
                       sys.executable, os.path.abspath(__file__), "--run", "--n", str(N), "--m", str(args.m), "--k", str(args.k),
                       "--t", str(args.t), "--ln-switch", str(args.ln_switch), "--reps", str(args.reps), "--warmup", str(args.warmup)]
                if body:
                    cmd += ["--body", body]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, cwd=ROOT)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    raise SystemExit(f"N = {N}: rocprofv3 run failed with status {r.returncode}")
                host = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                if "refused" in host:
                    ents[body] = host
                    continue
                traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
                if len(traces) != 1:
                    raise SystemExit(f"N = {N}: expected one kernel trace, found {traces}")
                k = kernel_ms(traces[0], args.warmup + args.reps, args.warmup, {"trans_posteriors": 1} if body else None)  # (the probe)
                for kind in k:
                    k[kind].update(host[kind])
                ent = dict(kinds=k)
                if all("kernel_ms" in k[kind] for kind in KINDS):
                    ent["over_posteriors"] = k["trans_posteriors"]["kernel_ms"] / k["posteriors"]["kernel_ms"]
                    ent["over_trans"] = k["trans_posteriors"]["kernel_ms"] / k["trans"]["kernel_ms"]
                    ent["over_posteriors_event"] = k["trans_posteriors"]["event_ms"] / k["posteriors"]["event_ms"]
                    ent["over_trans_event"] = k["trans_posteriors"]["event_ms"] / k["trans"]["event_ms"]
                ents[body] = ent
        if args.bodies:
            ms = {b: x["kinds"]["trans_posteriors"].get("kernel_ms") for b, x in ents.items() if "kinds" in x}
            if ms.get("looped") and ms.get("resident"):
                ents["looped_over_resident"] = ms["looped"] / ms["resident"]
        rec["by_N"][str(N)] = ents if args.bodies else ents[None]
        print(json.dumps({str(N): rec["by_N"][str(N)]}), flush=True)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
