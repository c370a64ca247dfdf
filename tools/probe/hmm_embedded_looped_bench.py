#!/usr/bin/env python3
"""Kernel time of the looped body of the embedded E-step (ECOZ2_HMM_EMBED_BODY), with the discipline of
hmm_embedded_bench.py: one stream of T symbols (M = 1024), models of N states, transcripts of L units cycling through 5
models, ln_switch = -1; HIP events around the kernels (embedded_last_kernel_ms / align_last_kernel_ms); `warmup` calls
discarded, then the median, least and greatest of `reps`.  Two tables:

  forced   the looped body forced at the four shapes hmm_embedded_bench.py records, against the resident body in the same
           process: the price of LDS-resident state and of the extra pass over the slots
  above    shapes of more than 16 slots, which only the looped body takes, against the alignment of the same stream to the
           same transcript (k_hmm_align's looped body): how many alignments the E-step costs.  Where the plan refuses the
           shape, the refusal is recorded instead of a time.

    python tools/probe/hmm_embedded_looped_bench.py [--out profiles/hmm_embedded_looped_bench.json] [--T 38265] [--reps 7] [--warmup 2]
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
FORCED = ((5, 20), (16, 20), (32, 20), (5, 100))
ABOVE = ((16, 100), (32, 100), (5, 500), (16, 500))


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
    ap.add_argument("--out", default="profiles/hmm_embedded_looped_bench.json")
    ap.add_argument("--T", type=int, default=38265)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    sym = rng.integers(0, M, a.T).astype(np.uint16)
    offs = np.array([0, a.T], dtype=np.int64)
    doc = dict(tool="tools/probe/hmm_embedded_looped_bench.py", M=M, K=K, T=a.T, ln_switch=LN_SWITCH, reps=a.reps, warmup=a.warmup,
               forced=[], above=[])

    def estep(models, units, L, body):
        got = {}
        t = timed(lambda: got.update(hmm.embedded_estep(models, sym, offs, units, [0, L], None, LN_SWITCH, body=body)),
                  hmm.embedded_last_kernel_ms, a.reps, a.warmup)
        t["status"] = int(got["status"][0])
        t["us_per_frame"] = 1e3 * t["kernel_ms"] / a.T
        return t, got

    for table, shapes in (("forced", FORCED), ("above", ABOVE)):
        for N, L in shapes:
            e.hmm.set_random_seed(N)
            models = [hmm.init_model(N, M, 0) for _ in range(K)]
            units = (np.arange(L) % K).astype(np.int32)
            row = dict(N=N, L=L, slots=slots_of([N] * L), sum_N=N * L)
            try:
                row["looped"], got = estep(models, units, L, "looped")
            except e.Ecoz2Error as err:
                row["refused"] = str(err)
            if table == "forced":
                row["resident"], ref = estep(models, units, L, "resident")
                row["same_words"] = bool(all(np.array_equal(x, y) for x, y in zip(got["acc"], ref["acc"])) and
                                         got["log_prob"].tobytes() == ref["log_prob"].tobytes())
                row["looped_over_resident"] = row["looped"]["kernel_ms"] / row["resident"]["kernel_ms"]
            else:
                al = {}
                row["align"] = timed(lambda: al.update(hmm.align(models, sym, offs, units, [0, L], None, LN_SWITCH)), hmm.align_last_kernel_ms,
                                     a.reps, a.warmup)
                if "looped" in row:
                    row["estep_over_align"] = row["looped"]["kernel_ms"] / row["align"]["kernel_ms"]
            print(json.dumps(row), flush=True)
            doc[table].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(a.out, "written")


if __name__ == "__main__":
    main()
