"""Measures the LPC front-end (`ecoz2 lpc`) on one GPU and prints one JSON record (optionally also written to --out).

  kernel   e2vq_lpc_analyze on one 32 kHz signal of >= 2^20 frames (P = 36, W = 45, O = 15): HIP-event kernel time,
           frames/s, executed FP64 operations 2 sum_i (win - i) + 4 win per frame against the FP64 VALU ceiling
           256 CUs x 64 lanes x 2.4 GHz (spec clock; the ceiling is not measured here)
  cpu      stand-in: the strict oracle's lpca (oracle/vq_oracle.c) on windowed frames, one thread per host core --
           not the reference's C (absent), and not its -ffast-math build
  e2e      `ecoz2 lpc` wall time on a warm-cache corpus of --files x --seconds, next to the time the library's own WAV
           reader and .prd writer take for the same files and bytes with the same reader threads (no analysis)
--kernel-only runs the kernel part alone (for a `rocprofv3 --kernel-trace --stats` run of its own).
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ecoz2rs_amd as e  # noqa: E402
from ecoz2rs_amd._lib import check  # noqa: E402
from tests import lpc_restatement as R  # noqa: E402
from tests import lpc_wavs  # noqa: E402

CEILING = 256 * 64 * 2.4e9  # FP64 VALU operations / s at the spec clock (unmeasured)


def sources_hash():
    h = hashlib.sha256()
    for f in ("lpc_device.hip", "lpc_device.h", "lpc_host.cpp"):
        h.update(open(os.path.join(ROOT, "ecoz2rs_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def host_cores():
    """Cores this process may use: the affinity mask, capped by a cgroup CPU quota when there is one."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def ops_per_frame(win, P):
    return 2 * sum(win - i for i in range(P + 1)) + 4 * win


def bench_kernel(frames_min, reps):
    sr, P = 32000, 36
    win, off = 45 * sr // 1000, 15 * sr // 1000
    N = (frames_min - 1) * off + win  # exactly frames_min frames
    s = np.random.default_rng(1).integers(-4000, 4000, N, dtype=np.int32)
    _w, _o, T = R.geometry(N, sr, 45, 15)
    frames = np.empty((T, P + 1))
    status = np.empty(T, dtype=np.int32)
    ms = []
    for _ in range(reps + 1):  # the first call is a warm-up
        Tc = C.c_int64()
        check(e.lib.e2vq_lpc_analyze(0, P, 45, 15, s.ctypes.data, N, sr, frames.ctypes.data, status.ctypes.data, T,
                                     C.byref(Tc), 0))
        k = C.c_float()
        check(e.lib.e2vq_lpc_last_kernel_ms(C.byref(k)))
        ms.append(k.value)
    ms = ms[1:]
    # spot check: a few frames against the restatement
    idx = [0, T // 2, T - 1]
    for t in idx:
        seg = s[t * off:t * off + win]
        f_r, st_r = R.analyze(seg, sr)
        assert st_r[0] == status[t] and np.array_equal(f_r[0].view(np.uint64), frames[t].view(np.uint64)), t
    best = min(ms)
    opf = ops_per_frame(win, P)
    return {"P": P, "sample_rate": sr, "win": win, "off": off, "frames": T, "kernel_ms": ms, "kernel_ms_min": best,
            "kernel_ms_median": float(np.median(ms)), "frames_per_s": T / (best * 1e-3),
            "fp64_ops_per_frame": opf, "fp64_ops_per_s": T * opf / (best * 1e-3),
            "fraction_of_fp64_valu_ceiling": T * opf / (best * 1e-3) / CEILING,
            "ceiling_ops_per_s_spec_unmeasured": CEILING, "target_fraction": 0.4}, s, frames, status


def bench_cpu(frames_cpu):
    from tests import oracle_lib

    o = oracle_lib.load()
    sr, P = 32000, 36
    off, win = 480, 1440
    N = (frames_cpu + 1) * off + win
    s = (np.random.default_rng(2).standard_normal(N) * 4000).astype(np.int32)
    w = R.windowed_frames(s, sr, 45, 15)
    cores = host_cores()
    chunks = np.array_split(np.arange(len(w)), cores)

    def run(ix):
        r, rc, a = np.zeros(P + 1), np.zeros(P + 1), np.zeros(P + 1)
        pe = C.c_double()
        for t in ix:
            x = w[t]
            o.L.e2o_lpca(x.ctypes.data, len(x), P, r.ctypes.data, rc.ctypes.data, a.ctypes.data, C.byref(pe))

    t0 = time.perf_counter()
    with ThreadPoolExecutor(cores) as ex:
        list(ex.map(run, chunks))
    dt = time.perf_counter() - t0
    return {"label": "CPU stand-in: strict oracle lpca (autocorrelation + Levinson only, frames pre-windowed), not the "
                     "reference's C", "host_cores": cores, "frames": len(w), "seconds": dt, "frames_per_s": len(w) / dt}


def bench_e2e(n_files, seconds):
    exe = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
    d = tempfile.mkdtemp(prefix="lpc_bench_")
    try:
        sr = 32000
        rng = np.random.default_rng(3)
        files = []
        base = rng.integers(-8000, 8000, sr * seconds, dtype=np.int32)
        for i in range(n_files):
            p = os.path.join(d, "signals", f"C{i % 10:02d}", f"{i:05d}.wav")
            lpc_wavs.write_wav(p, np.roll(base, int(rng.integers(0, len(base)))), sr, 16)
            files.append(p)
        total_bytes = sum(os.path.getsize(f) for f in files)
        for f in files:  # warm the page cache
            with open(f, "rb") as fh:
                while fh.read(1 << 24):
                    pass
        env = dict(os.environ, ECOZ2_VQ_OUT_ROOT=os.path.join(d, "out_lpc"))
        t0 = time.perf_counter()
        r = subprocess.run([exe, "lpc", "-P", "36", "-W", "45", "-O", "15", "--signals", os.path.join(d, "signals")],
                           env=env, capture_output=True, text=True, timeout=1800)
        t_lpc = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-2000:]
        # the baseline: same reader, same number of reader threads, same .prd bytes, no analysis (in-process: no
        # HIP start-up in it; the CLI's includes it)
        _w, _o, T = R.geometry(sr * seconds, sr, 45, 15)
        payload = np.zeros((T, 37))
        out = os.path.join(d, "out_base")
        threads = 4  # the reader threads of ecoz2_lpc_signals (e2vq_io::io_threads)

        def one(p):
            s, _ = e.lpc.wav_read(p)
            q = os.path.join(out, "data", "predictors", os.path.basename(os.path.dirname(p)),
                             os.path.basename(p)[:-4] + ".prd")
            check(e.lib.e2vq_prd_write(q.encode(), b"C", 36, payload.ctypes.data, T))
            return len(s)

        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, files))
        t_base = time.perf_counter() - t0
        # the entry point in this process (HIP already started by the kernel part): stdout to /dev/null
        os.environ["ECOZ2_VQ_OUT_ROOT"] = os.path.join(d, "out_warm")
        sys.stdout.flush()
        saved = os.dup(1)
        null = os.open(os.devnull, os.O_WRONLY)
        os.dup2(null, 1)
        try:
            t0 = time.perf_counter()
            e.lpc.lpc_signals(36, 45, 15, 0, 0.0, files, mintrpt=1e9)
            t_warm = time.perf_counter() - t0
        finally:
            os.dup2(saved, 1)
            os.close(null)
            os.close(saved)
            del os.environ["ECOZ2_VQ_OUT_ROOT"]
        return {"files": n_files, "seconds_per_file": seconds, "wav_bytes": total_bytes,
                "frames_total": T * n_files, "ecoz2_lpc_cli_wall_s": t_lpc,
                "ecoz2_lpc_signals_warm_s": t_warm, "read_write_baseline_s": t_base, "baseline_threads": threads,
                "ratio_cli": t_lpc / t_base, "ratio_warm_entry_point": t_warm / t_base, "target_ratio": 1.3,
                "lpc_stdout_tail": r.stdout.splitlines()[-2:]}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-frames", type=int, default=1 << 14)
    ap.add_argument("--files", type=int, default=200)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if e.lib.e2vq_device_count() < 1:
        raise SystemExit("lpc_bench: no HIP device")
    rec = {"sources": sources_hash()}
    rec["kernel"] = bench_kernel(a.frames, a.reps)[0]
    if not a.kernel_only:
        rec["cpu"] = bench_cpu(a.cpu_frames)
        rec["kernel"]["speedup_vs_cpu_stand_in"] = rec["kernel"]["frames_per_s"] / rec["cpu"]["frames_per_s"]
        rec["e2e"] = bench_e2e(a.files, a.seconds)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
