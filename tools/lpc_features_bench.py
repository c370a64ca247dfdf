"""Measures the LPC feature kernel (e2vq_lpc_features on device-resident frames) on one GPU; prints one JSON record
(optionally also written to --out).

For each order P (default 36, 12, 40) and Q = 48: --frames synthetic frames (2^16 distinct ones, tiled) as one
torch.float64 tensor on the device, every output requested (status, pe, rc, a, c).  Reported per order:
  kernel_ms      median HIP-event time of the kernel over --reps runs (after --warmup), and frames/s from it
  fp64           FP64 VALU operations per frame, counted as DESIGN.md section 8 does (one per IEEE add / sub / mul / neg;
                 an IEEE division is the 10 instructions of its expansion: 2 div_scale, rcp, 4 fma, mul, div_fmas,
                 div_fixup; the sqrt and log of c[0] are left out), against 256 CUs x 64 lanes x 2.4 GHz (spec clock)
  hbm            bytes read and written per frame against 6.3 TB/s (the measured copy bandwidth of the MI355X guide)
--kernel-only prints nothing but the record (for a `rocprofv3 --kernel-trace --stats` run of its own).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch.cuda.init()  # torch's HIP runtime first, then the library (as the torch tests do)

import ecoz2rs_amd as e  # noqa: E402
from ecoz2rs_amd._lib import check  # noqa: E402

FP64_CEILING = 256 * 64 * 2.4e9  # FP64 VALU instructions / s at the spec clock (not measured)
HBM = 6.3e12  # B / s, measured copy bandwidth (MI355X guide)
DIV = 10  # FP64 VALU instructions of one IEEE division


def ops_per_frame(P, Q):
    lev = sum(2 * k + DIV + 4 * (k >> 1) + 3 for k in range(1, P + 1))
    cep = 1  # c[1] = -a[1]
    cep += sum(3 * (i - 1) + 1 + DIV for i in range(2, P + 1))
    cep += sum(3 * P + 1 + DIV for i in range(P + 1, Q))
    return lev + cep


def bytes_per_frame(P, Q):
    NC = P + 1
    return NC * 8 + 4 + 8 + 2 * NC * 8 + Q * 8


def bench(P, Q, n, reps, warmup):
    base = e.synth.synth_frames(2024, 4, P, 0, 1 << 16)
    reps_needed = -(-n // len(base))
    x = torch.from_numpy(np.tile(base, (reps_needed, 1))[:n]).to("cuda")
    ms = C.c_float()
    times, walls = [], []
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        f = e.lpc.features(x, q=Q)
        walls.append(time.perf_counter() - t0)
        check(e.lib.e2vq_lpc_last_kernel_ms(C.byref(ms)))
        times.append(ms.value)
        if it == 0:
            st = f["status"].cpu().numpy()
            finite = bool(torch.isfinite(f["c"][:, 1:]).all())
        del f
    k = float(np.median(times[warmup:]))
    ops, nbytes = ops_per_frame(P, Q), bytes_per_frame(P, Q)
    fps = n / (k * 1e-3)
    return dict(P=P, Q=Q, frames=n, kernel_ms=round(k, 4), kernel_ms_min=round(min(times[warmup:]), 4),
                call_ms_median=round(1e3 * float(np.median(walls[warmup:])), 3), frames_per_s=round(fps),
                fp64_ops_per_frame=ops, fp64_fraction=round(fps * ops / FP64_CEILING, 4),
                bytes_per_frame=nbytes, hbm_fraction=round(fps * nbytes / HBM, 4),
                status_counts={int(s): int((st == s).sum()) for s in np.unique(st)}, c_finite=finite)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--orders", default="36,12,40")
    ap.add_argument("--q", type=int, default=48)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    rec = dict(tool="lpc_features_bench", device=torch.cuda.get_device_name(0), target_frames_per_s_P36=2e9,
               results=[bench(int(P), a.q, a.frames, a.reps, a.warmup) for P in a.orders.split(",")])
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
