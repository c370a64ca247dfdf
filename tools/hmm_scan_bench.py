#!/usr/bin/env python3
"""`hmm scan` against what a user can do without it -> profiles/hmm_scan_bench.json.

One stream of 38 265 symbols (the length of the reference's documented recording), M = 1024, K = 20 models, windows of
L = 100 symbols every H in {1, 10}, N in {5, 16, 32, 64}.  Per configuration:
  (a) e2vq_hmm_scan, top-2 output only: wall time of the call (upload of the 38 265 symbols included) and the HIP-event time
      of its kernels (e2vq_hmm_scan_last_kernel_ms), with the host's choice of body and with each body forced
      (ECOZ2_HMM_SCAN_PACK = 0 / 1);
  (b) the windows materialised as W separate sequences and scored by one e2vq_hmm_score call: wall time of the call (upload
      of the W x L symbols included; the materialisation itself is timed apart).  --baseline-lib names the library (b) runs
      on -- a build of the commit before `hmm scan` -- so that the baseline is never the code under test.  That library has
      no timer around k_hmm_score: its kernel time comes from a run of --arm b under `rocprofv3 --kernel-trace`, whose
      kernel_trace.csv --merge-trace reads (dispatches in configuration order, warm-up + repetitions per configuration).
Every arm is warmed up, repeated --reps times in alternation with the others, and reported as median with min and max.
(a)'s top-2 is checked against the argsort of (b)'s matrix before anything is timed."""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_STREAM, M, K, L = 38265, 1024, 20, 100
HOPS, NS = (1, 10), (5, 16, 32, 64)


def models_of(N, rng):
    row = lambda n: (lambda x: x / x.sum())(rng.uniform(0.05, 1.0, n))
    return [(row(N), np.stack([row(N) for _ in range(N)]), np.stack([row(M) for _ in range(N)])) for _ in range(K)]


def score_with(lib, models, sym, offs, S):
    ms = [tuple(np.ascontiguousarray(x) for x in m) for m in models]
    Ns = (C.c_int * K)(*[len(m[0]) for m in ms])
    ptr = lambda i: (C.c_void_p * K)(*[m[i].ctypes.data for m in ms])
    mant, ex = np.zeros((S, K)), np.zeros((S, K), dtype=np.int64)
    st, lp = np.zeros((S, K), dtype=np.int32), np.zeros((S, K))
    fn = lib.e2vq_hmm_score
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int] + [C.POINTER(C.c_void_p)] * 3 + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 4
    rc = fn(0, K, Ns, M, ptr(0), ptr(1), ptr(2), sym.ctypes.data, offs.ctypes.data, S, mant.ctypes.data, ex.ctypes.data,
            st.ctypes.data, lp.ctypes.data)
    if rc:
        raise RuntimeError("e2vq_hmm_score failed")
    return lp


def stats(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def merge_trace(doc, path, warmup, reps):
    rows = [r for r in csv.DictReader(open(path)) if "k_hmm_score" in r["Kernel_Name"]]
    per = warmup + 1 + reps  # (one more call per configuration: the parity check)
    assert len(rows) == per * len(doc["configs"]), (len(rows), per, len(doc["configs"]))
    for i, c in enumerate(doc["configs"]):
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows[i * per + warmup + 1:(i + 1) * per]]
        c["b_kernel_ms"] = stats(ms)
        c["kernel_ratio_b_over_a"] = c["b_kernel_ms"]["median"] / c["a_kernel_ms"]["median"]
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", help="libecoz2vq.so of the commit before hmm scan (default: this tree's library)")
    ap.add_argument("--arm", choices=("all", "b"), default="all", help="b: only the baseline calls (for a kernel trace)")
    ap.add_argument("--merge-trace", help="kernel_trace.csv of an --arm b run: adds (b)'s kernel times to --out and exits")
    ap.add_argument("--ns", help="comma-separated N instead of 5,16,32,64 (the cutoff between the bodies)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmm_scan_bench.json"))
    a = ap.parse_args()
    if a.merge_trace:
        doc = merge_trace(json.load(open(a.out)), a.merge_trace, a.warmup, a.reps)
        json.dump(doc, open(a.out, "w"), indent=1)
        return
    import ecoz2rs_amd as e
    from ecoz2rs_amd import hmm

    if e.lib.e2vq_device_count() < 1:
        raise SystemExit("hmm_scan_bench needs a HIP device")
    base = C.CDLL(a.baseline_lib) if a.baseline_lib else e.lib
    rng = np.random.default_rng(2024)
    stream = rng.integers(0, M, T_STREAM).astype(np.uint16)
    offs1 = np.array([0, T_STREAM], dtype=np.int64)
    doc = dict(stream=T_STREAM, M=M, K=K, L=L, reps=a.reps, warmup=a.warmup,
               baseline_lib="parent commit" if a.baseline_lib else "this tree", configs=[])
    arms = {"a": None, "a_pack0": "0", "a_pack1": "1"}
    for N in ([int(x) for x in a.ns.split(",")] if a.ns else NS):
        models = models_of(N, rng)
        for H in HOPS:
            t0 = time.perf_counter()
            idx = np.arange(0, T_STREAM - L + 1, H)[:, None] + np.arange(L)[None, :]
            wsym = np.ascontiguousarray(stream[idx].ravel())
            woffs = np.arange(len(idx) + 1, dtype=np.int64) * L
            materialise_ms = (time.perf_counter() - t0) * 1e3
            W = len(idx)

            def run_b():
                t = time.perf_counter()
                lp = score_with(base, models, wsym, woffs, W)
                return (time.perf_counter() - t) * 1e3, lp

            def run_a(pack):
                if pack is None:
                    os.environ.pop("ECOZ2_HMM_SCAN_PACK", None)
                else:
                    os.environ["ECOZ2_HMM_SCAN_PACK"] = pack
                t = time.perf_counter()
                got = hmm.scan(models, stream, offs1, L, H, matrix=False)
                return (time.perf_counter() - t) * 1e3, hmm.scan_last_kernel_ms(), got

            for _ in range(a.warmup):
                run_b()
            _ms, lp = run_b()
            c = dict(N=N, H=H, W=W, materialise_ms=materialise_ms)
            if a.arm == "all":
                order = np.argsort(lp, axis=1, kind="stable")
                for pack in arms.values():
                    for _ in range(a.warmup):
                        run_a(pack)
                    got = run_a(pack)[2]
                    assert np.array_equal(got["best"], order[:, -1]) and np.array_equal(got["second"], order[:, -2])
            wall = {k: [] for k in ("b", *arms)}
            kern = {k: [] for k in arms}
            for _ in range(a.reps):  # alternating
                wall["b"].append(run_b()[0])
                if a.arm == "all":
                    for name, pack in arms.items():
                        w, km, _g = run_a(pack)
                        wall[name].append(w)
                        kern[name].append(km)
            c["b_wall_ms"] = stats(wall["b"])
            if a.arm == "all":
                for name in arms:
                    c[name + "_wall_ms"] = stats(wall[name])
                    c[name + "_kernel_ms"] = stats(kern[name])
                c["wall_ratio_b_over_a"] = c["b_wall_ms"]["median"] / c["a_wall_ms"]["median"]
            doc["configs"].append(c)
            print(json.dumps(c), flush=True)
    if a.arm == "all":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(doc, open(a.out, "w"), indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
