"""Measures the streaming decoder of `hmm segment --class-transitions --grammar-continuous` against one
`hmm segment --class-transitions` call on the same models, prices and stream: what decoding block by block costs under a
matrix of prices, and what it saves in device memory.  Prints one JSON record (optionally also written to --out).

The workload is tools/hmm_segment_trans_bench.py's (4.8.8): one stream of --t random symbols (default 38 265), M = 1024, K = 20
random models of N states each, the planted matrix plus --ln-switch (default -5).  Per N (default 5, 16, 32), --warmup +
--reps of each:
  comparator   one e2vq_hmm_segment_trans call on the whole stream: e2vq_hmm_segment_trans_last_kernel_ms and the call's wall
               time
  stream_B     a matrix session with blocks of B frames (default 4096 and 512), opened outside the timed part, fed the whole
               stream in one feed and closed: e2vq_hmm_segment_stream_kernel_ms (the HIP-event time of all its kernels), the
               part of it spent in coalescence and backtrack, and the wall time of feed + close + take
Times are HIP-event times of the calls themselves: median and min .. max over the repetitions.  per_block_ms = (stream_512 -
stream_4096) / (difference in block count), the fixed cost of a block (launch, lA and lt staged again).  ratio = stream_4096 /
comparator of the medians.  Also recorded: the most frames pending at once, and the device bytes of the session (measured
under a pending budget of 64 MiB, --pending-bytes) next to the one-shot tables of T (2 sum N + 12 K) bytes.
--bodies (a list of auto, resident, looped: ECOZ2_HMM_SEGMENT_TRANS_BODY of the one-shot calls and of the sessions' open): a run
per N and body, by_N[N][body], and looped_over_resident (the sessions at the first block length) where both ran.  A packing the
body refuses (more than 16 wave-slots under resident) is recorded as refused, with the library's message.  Without it, one run
per N with the environment's body, by_N[N], as before.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def stats(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="5,16,32")
    ap.add_argument("--blocks", default="4096,512")
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--t", type=int, default=38265)
    ap.add_argument("--ln-switch", type=float, default=-5.0)
    ap.add_argument("--pending-bytes", type=int, default=64 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bodies", help="auto, resident and / or looped, comma-separated: a run per N and body")
    ap.add_argument("--out")
    args = ap.parse_args()
    import numpy as np

    import ecoz2rs_amd as e
    from hmm_segment_trans_bench import workload

    keys = ("cls", "state", "entered")
    blocks = [int(x) for x in args.blocks.split(",")]
    rec = dict(tool="tools/hmm_segment_trans_stream_bench.py", M=args.m, K=args.k, T=args.t, ln_switch=args.ln_switch, reps=args.reps,
               warmup=args.warmup, pending_bytes=args.pending_bytes, by_N={})
    os.environ["ECOZ2_HMM_SEGMENT_STREAM_PENDING_BYTES"] = str(args.pending_bytes)
    bodies = args.bodies.split(",") if args.bodies else [None]
    if args.bodies:
        rec["bodies"] = bodies

    def measure(N, models, sym, lt, body):
        offs = np.array([0, args.t], dtype=np.int64)
        try:
            e.hmm.segment_trans(models, sym[:8], [0, 8], lt, body=body)
        except e.Ecoz2Error as err:
            return dict(refused=str(err))
        ent = {}
        ev, wall = [], []
        for _ in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            want = e.hmm.segment_trans(models, sym, offs, lt, body=body)
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(e.hmm.segment_trans_last_kernel_ms())
        ent["comparator"] = dict(kernel_ms=stats(ev[args.warmup:]), call_wall_ms=stats(wall[args.warmup:]),
                                 table_bytes=args.t * (2 * N * args.k + 12 * args.k))
        for B in blocks:
            os.environ["ECOZ2_HMM_SEGMENT_STREAM_BLOCK"] = str(B)
            ev, cm, wall = [], [], []
            for _ in range(args.warmup + args.reps):
                with e.hmm.SegmentTransStream(models, lt, body=body) as s:
                    t0 = time.perf_counter()
                    a = s.feed(sym)
                    b = s.close()
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ev.append(s.kernel_ms())
                    st = s.stats()
                    cm.append(st["commit_ms"])
                    same = all(np.array_equal(np.concatenate([a[k], b[k]]), want[k]) for k in keys) and \
                        np.array_equal(np.concatenate([a["exit_score"], b["exit_score"]]).view(np.uint64), want["exit_score"].view(np.uint64)) and \
                        s.log_prob == want["log_prob"][0]
                    if not same:
                        raise SystemExit(f"N = {N}, B = {B}: the session differs from the one-shot decode")
            ent[f"stream_{B}"] = dict(kernel_ms=stats(ev[args.warmup:]), commit_ms=stats(cm[args.warmup:]),
                                      commit_share=statistics.median(cm[args.warmup:]) / statistics.median(ev[args.warmup:]),
                                      call_wall_ms=stats(wall[args.warmup:]), blocks=-(-args.t // B), peak_pending=st["peak_pending"],
                                      final_after_feed=len(a["cls"]), device_bytes=st["device_bytes"])
        c = ent["comparator"]["kernel_ms"]
        ent["ratio"] = ent[f"stream_{blocks[0]}"]["kernel_ms"]["median"] / c["median"]
        if len(blocks) >= 2:
            hi, lo = ent[f"stream_{blocks[0]}"], ent[f"stream_{blocks[1]}"]
            ent.update(per_block_ms=(lo["kernel_ms"]["median"] - hi["kernel_ms"]["median"]) / (lo["blocks"] - hi["blocks"]),
                       ratio_small_blocks=lo["kernel_ms"]["median"] / c["median"])
        return ent

    for N in [int(x) for x in args.ns.split(",")]:
        models, sym, lt = workload(N, args.m, args.k, args.t, args.ln_switch)
        ents = {body: measure(N, models, sym, lt, body) for body in bodies}
        if args.bodies:
            ms = {b: x[f"stream_{blocks[0]}"]["kernel_ms"]["median"] for b, x in ents.items() if "refused" not in x}
            if ms.get("looped") and ms.get("resident"):
                ents["looped_over_resident"] = ms["looped"] / ms["resident"]
        rec["by_N"][str(N)] = ents if args.bodies else ents[None]
        print(json.dumps({str(N): rec["by_N"][str(N)]}), flush=True)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
