#!/usr/bin/env python3
"""Kernel time of the alignment posteriors against two comparators in the same process: the alignment of the
same stream to the same transcript (k_hmm_align and its backtrack) and the embedded E-step (k_hmm_embed_fb), whose forward pass
the posteriors share and whose backward pass they run without xi, limbs and atomics.  The expectation this records is that the
posteriors lie between the two; it is an expectation, not a threshold.

One stream of T symbols (M = 1024), models of N states, transcripts of L units cycling through 5 models, ln_switch = -1 (the
method of tools/probe/hmm_embedded_bench.py).  Every time is the HIP-event pair around the kernels of a call
(align_posteriors_last_kernel_ms / align_last_kernel_ms / embedded_last_kernel_ms); no trace, no counters.  The posteriors run
with the path and the begin frames of the alignment, once with the occupancy table (T x L doubles) and once without.  `warmup`
calls discarded, then the median, least and greatest of `reps`.

Two more tables for the looped body (ECOZ2_HMM_ALIGN_POSTERIOR_BODY, hmm_align_posterior_looped.hip):

  forced   the looped body forced at the four shapes above, against the resident body in the same process (the two alternate
           call by call): the price of LDS-resident state and of the extra pass over the slots, which `auto` avoids
  above    the long-transcript rows of 4.8.10 (more than 16 slots, which only the looped body takes): the looped posteriors
           against the looped E-step (k_hmm_embed_fb_looped) and the alignment of the same stream to the same transcript, the
           three alternating call by call.  The posteriors do a subset of the E-step's work, so over_estep should not exceed 1
           beyond the spread of the runs; over_estep_min / _max are the least and greatest ratio of a pair of neighbouring calls.

    python tools/probe/hmm_align_posteriors_bench.py [--out profiles/hmm_align_posteriors_bench.json] [--T 38265] [--reps 7]
                                                     [--warmup 2]
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
SHAPES = ((5, 20), (16, 20), (32, 20), (5, 100))
ABOVE = ((5, 500), (16, 500), (16, 100), (32, 100))


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


def alternating(calls, reps, warmup):
    """calls: {key: (call, last_ms)}, run one after the other `warmup` + `reps` times -> ({key: the summary of `timed`}, {key: [ms]})"""
    ms = {k: [] for k in calls}
    for r in range(warmup + reps):
        for k, (call, last_ms) in calls.items():
            call()
            if r >= warmup:
                ms[k].append(last_ms())
    return {k: dict(kernel_ms=statistics.median(v), kernel_ms_min=min(v), kernel_ms_max=max(v)) for k, v in ms.items()}, ms


def ratio(ms, a, b):
    """a over b: of the medians, and the least and greatest over the pairs of neighbouring calls"""
    pairs = [x / y for x, y in zip(ms[a], ms[b])]
    return statistics.median(ms[a]) / statistics.median(ms[b]), min(pairs), max(pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/hmm_align_posteriors_bench.json")
    ap.add_argument("--T", type=int, default=38265)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    sym = rng.integers(0, M, a.T).astype(np.uint16)
    offs = np.array([0, a.T], dtype=np.int64)
    doc = dict(tool="tools/probe/hmm_align_posteriors_bench.py", M=M, K=K, T=a.T, ln_switch=LN_SWITCH, reps=a.reps, warmup=a.warmup,
               shapes=[], forced=[], above=[])

    def setup(N, L):
        e.hmm.set_random_seed(N)
        models = [hmm.init_model(N, M, 0) for _ in range(K)]
        units = (np.arange(L) % K).astype(np.int32)
        return models, units, dict(N=N, L=L, slots=slots_of([N] * L), sum_N=N * L)

    def post(models, units, L, path, ref, body, occupancy, into):
        return lambda: into.update(hmm.align_posteriors(models, sym, offs, units, [0, L], None, LN_SWITCH, path_unit=path, ref=ref,
                                                        occupancy=occupancy, body=body))

    same = lambda x, y, keys: bool(all(np.array_equal(np.asarray(x[k]).view(np.uint64), np.asarray(y[k]).view(np.uint64)) for k in keys))
    for N, L in SHAPES:
        e.hmm.set_random_seed(N)
        models = [hmm.init_model(N, M, 0) for _ in range(K)]
        units = (np.arange(L) % K).astype(np.int32)
        uoffs = [0, L]
        row = dict(N=N, L=L, slots=slots_of([N] * L), sum_N=N * L)
        al, es, po = {}, {}, {}
        row["align"] = timed(lambda: al.update(hmm.align(models, sym, offs, units, uoffs, None, LN_SWITCH)), hmm.align_last_kernel_ms,
                             a.reps, a.warmup)
        row["estep"] = timed(lambda: es.update(hmm.embedded_estep(models, sym, offs, units, uoffs, None, LN_SWITCH)),
                             hmm.embedded_last_kernel_ms, a.reps, a.warmup)
        path, ref = al["unit"], np.where(al["begin"] < 0, 0, al["begin"])
        for key, occupancy in (("posteriors", False), ("posteriors_occ", True)):
            row[key] = timed(lambda: po.update(hmm.align_posteriors(models, sym, offs, units, uoffs, None, LN_SWITCH, path_unit=path, ref=ref,
                                                                    occupancy=occupancy)),
                             hmm.align_posteriors_last_kernel_ms, a.reps, a.warmup)
            row[key]["us_per_frame"] = 1e3 * row[key]["kernel_ms"] / a.T
            row[key]["over_align"] = row[key]["kernel_ms"] / row["align"]["kernel_ms"]
            row[key]["over_estep"] = row[key]["kernel_ms"] / row["estep"]["kernel_ms"]
        row["status"] = [int(al["status"][0]), int(es["status"][0]), int(po["status"][0])]
        row["same_log_prob_bits"] = bool(np.array_equal(es["log_prob"].view(np.uint64), po["log_prob"].view(np.uint64)))
        row["mean_post_path"] = float(po["post_path"].mean())
        row["between"] = bool(row["align"]["kernel_ms"] <= row["posteriors_occ"]["kernel_ms"] <= row["estep"]["kernel_ms"])
        print(json.dumps(row), flush=True)
        doc["shapes"].append(row)
    ms_of = hmm.align_posteriors_last_kernel_ms
    for N, L in SHAPES:
        models, units, row = setup(N, L)
        al = hmm.align(models, sym, offs, units, [0, L], None, LN_SWITCH)
        path, ref = al["unit"], np.where(al["begin"] < 0, 0, al["begin"])
        lo, re = {}, {}
        t, ms = alternating(dict(looped=(post(models, units, L, path, ref, "looped", True, lo), ms_of),
                                 resident=(post(models, units, L, path, ref, "resident", True, re), ms_of)), a.reps, a.warmup)
        row.update(t)
        row["looped_over_resident"], row["looped_over_resident_min"], row["looped_over_resident_max"] = ratio(ms, "looped", "resident")
        row["same_words"] = same(lo, re, ("post_path", "w0", "w1", "w2", "log_prob")) and same(lo["occ"], re["occ"], (0,))
        print(json.dumps(row), flush=True)
        doc["forced"].append(row)
    for N, L in ABOVE:
        models, units, row = setup(N, L)
        al, es, po, pn = {}, {}, {}, {}
        al.update(hmm.align(models, sym, offs, units, [0, L], None, LN_SWITCH))
        path, ref = al["unit"], np.where(al["begin"] < 0, 0, al["begin"])
        t, ms = alternating(dict(
            estep=(lambda: es.update(hmm.embedded_estep(models, sym, offs, units, [0, L], None, LN_SWITCH, body="auto")),
                   hmm.embedded_last_kernel_ms),
            posteriors_occ=(post(models, units, L, path, ref, "auto", True, po), ms_of),
            posteriors=(post(models, units, L, path, ref, "auto", False, pn), ms_of),
            align=(lambda: al.update(hmm.align(models, sym, offs, units, [0, L], None, LN_SWITCH)), hmm.align_last_kernel_ms)),
            a.reps, a.warmup)
        row.update(t)
        for key in ("posteriors", "posteriors_occ"):
            row[key]["us_per_frame"] = 1e3 * row[key]["kernel_ms"] / a.T
            row[key]["over_estep"], row[key]["over_estep_min"], row[key]["over_estep_max"] = ratio(ms, key, "estep")
            row[key]["over_align"], row[key]["over_align_min"], row[key]["over_align_max"] = ratio(ms, key, "align")
        row["status"] = [int(al["status"][0]), int(es["status"][0]), int(po["status"][0])]
        row["same_log_prob_bits"] = same(es, po, ("log_prob",))
        # (a random stream does not fit a transcript of hundreds of units: where bh overflows the contract's products are inf or
        # 0 x inf; the time of the arithmetic is what is measured, the frames are counted)
        finite = np.isfinite(po["post_path"])
        row["post_path_not_finite"] = int((~finite).sum())
        row["mean_post_path"] = float(po["post_path"][finite].mean()) if finite.any() else None
        print(json.dumps(row), flush=True)
        doc["above"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(a.out, "written")


if __name__ == "__main__":
    main()
