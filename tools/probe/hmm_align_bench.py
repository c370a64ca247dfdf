#!/usr/bin/env python3
"""Kernel time of `hmm align` against the only earlier route to an alignment: e2vq_hmm_segment_trans with
every transcript position posing as a class of its own under a chain-shaped price matrix.

One stream of T symbols (M = 1024), models of N states, transcripts of L units cycling through 5 models.  Times are HIP
events around the forward kernel and the backtrack (align_last_kernel_ms / segment_trans_last_kernel_ms): `warmup` calls
discarded, then the median, least and greatest of `reps`.  The baseline exists only where the L posed classes pack into 16
wave-slots; a shape that e2vq_hmm_align refuses is recorded with its message.

    python tools/probe/hmm_align_bench.py [--out profiles/hmm_align_bench.json] [--T 38265] [--reps 7] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import ecoz2rs_amd as e  # noqa: E402
from ecoz2rs_amd import hmm  # noqa: E402

M, K, LN_SWITCH = 1024, 5, -1.0


def slots_of(Ns):
    slots, fill = 0, 64
    for N in Ns:
        if fill + N > 64:
            slots, fill = slots + 1, 0
        fill += N
    return slots


def timed(call, last_ms, reps, warmup):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(reps):
        call()
        ms.append(last_ms())
    return dict(kernel_ms=statistics.median(ms), kernel_ms_min=min(ms), kernel_ms_max=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/hmm_align_bench.json")
    ap.add_argument("--T", type=int, default=38265)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    sym = rng.integers(0, M, a.T).astype(np.uint16)
    offs = np.array([0, a.T], dtype=np.int64)
    doc = dict(tool="tools/probe/hmm_align_bench.py", M=M, K=K, T=a.T, ln_switch=LN_SWITCH, reps=a.reps, warmup=a.warmup, shapes=[])
    for N in (5, 16, 32):
        e.hmm.set_random_seed(N)
        models = [hmm.init_model(N, M, 0) for _ in range(K)]
        for L in (20, 100, 500):
            units = (np.arange(L) % K).astype(np.int32)
            slots = slots_of([N] * L)
            row = dict(N=N, L=L, slots=slots, sum_N=N * L, body="resident" if slots <= 16 else "looped")
            try:
                got = {}
                row["align"] = timed(lambda: got.update(hmm.align(models, sym, offs, units, [0, L], None, LN_SWITCH)),
                                     hmm.align_last_kernel_ms, a.reps, a.warmup)
                row["align"]["status"] = int(got["status"][0])
                row["align"]["us_per_frame"] = 1e3 * row["align"]["kernel_ms"] / a.T
                row["align"]["ns_per_frame_and_slot"] = 1e6 * row["align"]["kernel_ms"] / a.T / slots
            except e.Ecoz2Error as err:
                row["align"] = dict(refused=str(err))
            if slots <= 16:  # the baseline: L posed classes, the price of f -> f + 1 alone finite
                lt = np.full((L, L), -np.inf)
                lt[np.arange(L - 1), np.arange(1, L)] = LN_SWITCH
                posed = [models[k] for k in units]
                row["baseline"] = timed(lambda: hmm.segment_trans(posed, sym, offs, lt), hmm.segment_trans_last_kernel_ms, a.reps, a.warmup)
                if "kernel_ms" in row["align"]:
                    row["align_over_baseline"] = row["align"]["kernel_ms"] / row["baseline"]["kernel_ms"]
            print(json.dumps(row), flush=True)
            doc["shapes"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(a.out, "written")


if __name__ == "__main__":
    main()
