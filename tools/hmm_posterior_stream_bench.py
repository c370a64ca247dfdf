"""Measures `hmm segment --continuous-posteriors` next to the closed pass it restates, on the same models
and stream in the same process; prints one JSON record (optionally also written to --out).

Cost.  The workload of tools/hmm_posteriors_bench.py: one stream of --t random symbols (default 38 265), M = 1024, K = 20
random models (e2vq_hmm_init type 0) of N states each, ln_switch = -5; per N (default 5, 16, 32, and 64 under the body
`auto`):
  closed     one e2vq_hmm_segment_posteriors call on the whole stream (its code is the parent commit's: the comparator)
  session    one posterior session fed the whole stream in one feed and closed, per (B, L) of --shapes (default
             4096:0, 4096:1024, 4096:4096 and 512:0 -- the last one to split the per-block cost from the spread)
--warmup + --reps of each, median and min .. max.  Times are the calls' own HIP-event times (`kernel_ms`: for a session,
first launch to last, the copies between them included) and the wall time of the whole call (`call_wall_ms`: for a session
open, feed, close and free).  `over_closed` = session / closed of the kernel medians.

What the look-ahead buys (--lookahead-table).  On the planted stream of the segment tests and on the stream above at --table-n
states, the worst and the mean |streamed - closed| posterior over all frames and classes for L in --table-ls at B = --table-b
(the planted stream has 510 frames: B = --planted-b, and every L >= 510 is the closed pass).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(N, M, K, T, seed=2026):
    import numpy as np

    import ecoz2rs_amd as e

    e.hmm.set_random_seed(seed + N)
    models = [e.hmm.init_model(N, M, 0) for _ in range(K)]
    sym = np.random.default_rng(seed).integers(0, M, T).astype(np.uint16)
    return models, sym


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def session(models, sym, ls, B, L, body):
    """-> (post, log_prob, kernel_ms, stats) of one session fed whole"""
    import numpy as np

    import ecoz2rs_amd as e

    with e.hmm.PosteriorStream(models, ls, block=B, lookahead=L, body=body) as s:
        parts = [s.feed(sym)[1], s.close()[1]]
        return np.concatenate(parts), s.log_prob, s.kernel_ms(), s.stats()


def cost(args, N, body):
    import numpy as np

    import ecoz2rs_amd as e

    models, sym = workload(N, args.m, args.k, args.t)
    offs = np.array([0, len(sym)], dtype=np.int64)
    n = args.warmup + args.reps
    ent = dict(body=body or "resident")
    wall, ev = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        closed = e.hmm.segment_posteriors(models, sym, offs, args.ln_switch, body=body)
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(e.hmm.segment_posteriors_last_kernel_ms())
    ent["closed"] = dict(kernel_ms=spread(ev[args.warmup:]), call_wall_ms=spread(wall[args.warmup:]))
    ent["sessions"] = {}
    for shape in args.shapes.split(","):
        B, L = (int(x) for x in shape.split(":"))
        wall, ev = [], []
        for _ in range(n):
            t0 = time.perf_counter()
            post, lp, ms, stats = session(models, sym, args.ln_switch, B, L, body)
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(ms)
        diff = np.abs(post - closed["post"])
        ent["sessions"][shape] = dict(
            kernel_ms=spread(ev[args.warmup:]), call_wall_ms=spread(wall[args.warmup:]),
            over_closed=statistics.median(ev[args.warmup:]) / ent["closed"]["kernel_ms"]["median"], launches=stats["launches"],
            backward_frames=stats["backward_frames"], device_bytes=stats["device_bytes"], ring_rows=stats["ring_rows"],
            log_prob_bits_equal=bool(np.float64(lp).view(np.uint64) == np.float64(closed["log_prob"][0]).view(np.uint64)),
            worst_abs_diff=float(diff.max()), mean_abs_diff=float(diff.mean()))
    return ent


def lookahead_table(args):
    import numpy as np

    import ecoz2rs_amd as e
    from tests.test_hmm_segment_stream_cpu import planted_models, planted_stream

    out = {}
    pm = planted_models()
    streams = {"planted": (pm, planted_stream(pm, np.random.default_rng(3)), -5.0, args.planted_b),
               "bench": workload(args.table_n, args.m, args.k, args.t) + (args.ln_switch, args.table_b)}
    for name, (models, sym, ls, B) in streams.items():
        closed = e.hmm.segment_posteriors(models, sym, [0, len(sym)], ls)["post"]
        rows = {}
        for L in [int(x) for x in args.table_ls.split(",")]:
            post = session(models, sym, ls, B, L, None)[0]
            diff = np.abs(post - closed)
            rows[str(L)] = dict(worst=float(diff.max()), mean=float(diff.mean()), frames_differing=int((diff.max(axis=1) > 0).sum()))
        out[name] = dict(T=len(sym), K=len(models), B=B, ln_switch=ls, by_L=rows)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="5,16,32,64")
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--t", type=int, default=38265)
    ap.add_argument("--ln-switch", type=float, default=-5.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="4096:0,4096:1024,4096:4096,512:0")
    ap.add_argument("--lookahead-table", action="store_true")
    ap.add_argument("--table-n", type=int, default=5)
    ap.add_argument("--table-b", type=int, default=4096)
    ap.add_argument("--planted-b", type=int, default=64)
    ap.add_argument("--table-ls", default="0,16,64,256,1024,4096")
    ap.add_argument("--out")
    args = ap.parse_args()
    rec = dict(tool="tools/hmm_posterior_stream_bench.py", M=args.m, K=args.k, T=args.t, ln_switch=args.ln_switch, reps=args.reps,
               warmup=args.warmup, timing="HIP events of the calls themselves, and wall time", by_N={})
    for N in [int(x) for x in args.ns.split(",") if x]:
        slots = -(-args.k // (64 // N))
        rec["by_N"][str(N)] = cost(args, N, "auto" if slots > 16 else None)
        print(json.dumps({str(N): rec["by_N"][str(N)]}), flush=True)
    if args.lookahead_table:
        rec["lookahead"] = lookahead_table(args)
        print(json.dumps(rec["lookahead"]), flush=True)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
