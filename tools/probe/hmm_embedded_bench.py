#!/usr/bin/env python3
"""Kernel time of the embedded E-step against two comparators in the same process: the alignment of the
same stream to the same transcript (how many alignments an E-step costs), and one iteration of the only route to a retrained
model there was before -- align, cut the stream at the boundaries, one E-step of e2vq_hmm_train_classes on the pieces.  That
route is another algorithm (hard boundaries), so its ratio compares costs and claims no speed-up.

One stream of T symbols (M = 1024), models of N states, transcripts of L units cycling through 5 models.  The E-step's and
the alignment's times are HIP events around their kernels (embedded_last_kernel_ms / align_last_kernel_ms); the cut-and-train
route has no event pair of its own and is timed by the host clock around calls that end in a device synchronise (the
alignment, the cut on the host, train_classes with max_iterations = 1: its upload and download included).  `warmup` calls
discarded, then the median, least and greatest of `reps`.

    python tools/probe/hmm_embedded_bench.py [--out profiles/hmm_embedded_bench.json] [--T 38265] [--reps 7] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import ecoz2rs_amd as e  # noqa: E402
from ecoz2rs_amd import hmm  # noqa: E402

M, K, LN_SWITCH = 1024, 5, -1.0
SHAPES = ((5, 20), (16, 20), (32, 20), (5, 100))


def slots_of(Ns):
    slots, fill = 0, 64
    for N in Ns:
        if fill + N > 64:
            slots, fill = slots + 1, 0
        fill += N
    return slots


def spread(ms, key):
    return {key: statistics.median(ms), key + "_min": min(ms), key + "_max": max(ms)}


def timed(call, last_ms, reps, warmup):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(reps):
        call()
        ms.append(last_ms())
    return spread(ms, "kernel_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/hmm_embedded_bench.json")
    ap.add_argument("--T", type=int, default=38265)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    sym = rng.integers(0, M, a.T).astype(np.uint16)
    offs = np.array([0, a.T], dtype=np.int64)
    doc = dict(tool="tools/probe/hmm_embedded_bench.py", M=M, K=K, T=a.T, ln_switch=LN_SWITCH, reps=a.reps, warmup=a.warmup, shapes=[])
    for N, L in SHAPES:
        e.hmm.set_random_seed(N)
        models = [hmm.init_model(N, M, 0) for _ in range(K)]
        units = (np.arange(L) % K).astype(np.int32)
        row = dict(N=N, L=L, slots=slots_of([N] * L), sum_N=N * L)
        got = {}
        row["estep"] = timed(lambda: got.update(hmm.embedded_estep(models, sym, offs, units, [0, L], None, LN_SWITCH)),
                             hmm.embedded_last_kernel_ms, a.reps, a.warmup)
        row["estep"]["status"] = int(got["status"][0])
        row["estep"]["us_per_frame"] = 1e3 * row["estep"]["kernel_ms"] / a.T
        al = {}
        row["align"] = timed(lambda: al.update(hmm.align(models, sym, offs, units, [0, L], None, LN_SWITCH)), hmm.align_last_kernel_ms,
                             a.reps, a.warmup)
        row["estep_over_align"] = row["estep"]["kernel_ms"] / row["align"]["kernel_ms"]

        def cut_and_train():
            r = hmm.align(models, sym, offs, units, [0, L], None, LN_SWITCH)
            pieces = [[] for _ in range(K)]
            for k, b, en in zip(units, r["begin"], r["end"]):
                if b >= 0:
                    pieces[k].append(sym[b:en])
            hmm.train_classes(models, pieces, max_iterations=1)

        for _ in range(a.warmup):
            cut_and_train()
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            cut_and_train()
            wall.append(1e3 * (time.perf_counter() - t0))
        row["cut_and_train"] = spread(wall, "wall_ms")
        wall = []
        for _ in range(a.reps):  # the E-step's own call by the same clock, for a like-for-like ratio
            t0 = time.perf_counter()
            hmm.embedded_estep(models, sym, offs, units, [0, L], None, LN_SWITCH)
            wall.append(1e3 * (time.perf_counter() - t0))
        row["estep"].update(spread(wall, "wall_ms"))
        row["estep_wall_over_cut_and_train_wall"] = row["estep"]["wall_ms"] / row["cut_and_train"]["wall_ms"]
        print(json.dumps(row), flush=True)
        doc["shapes"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(a.out, "written")


if __name__ == "__main__":
    main()
