"""LPC front-end: ``ecoz2 lpc`` (.wav -> .prd) and the analysis of signals already in memory, on the GPU.

Mirrors ``ecoz2_lib::lpc_signals`` (/root/reference/src/ecoz2_lib/mod.rs:193-218) and ``ecoz2_lib::lpca_c::lpca``
(src/ecoz2_lib/lpca_c.rs:19-37).  The arithmetic is the reference's Rust analysis (src/lpc/lpc_rs.rs, lpca_rs.rs:28-75),
bit for bit.
"""
import ctypes as C

import numpy as np

from ._lib import check, lib
from .vq import _to_vec_of_ptr_const_c_char


def lpc_signals(prediction_order, window_length_ms, offset_length_ms, minpc, split, sgn_filenames, mintrpt=5.0,
                verbose=False):
    """Writes data/predictors/<class>/<stem>.prd for every .wav (class = name of its parent directory)."""
    files, _keep = _to_vec_of_ptr_const_c_char(sgn_filenames)
    check(lib.ecoz2_lpc_signals(int(prediction_order), int(window_length_ms), int(offset_length_ms), int(minpc),
                                float(split), files, len(sgn_filenames), float(mintrpt), int(bool(verbose))))


def frame_count(num_samples, sample_rate, W=45, O=15):
    """(win, off, T) of src/lpc/lpc_rs.rs:203-218; T = -1 for a signal shorter than one window."""
    win, off, T = C.c_int(), C.c_int(), C.c_int64()
    check(lib.e2vq_lpc_frame_count(int(num_samples), int(sample_rate), int(W), int(O), C.byref(win), C.byref(off),
                                   C.byref(T)))
    return win.value, off.value, T.value


def wav_info(path):
    """(sample_rate, num_samples, bits_per_sample) of a mono integer-PCM .wav."""
    sr, n, bits = C.c_int(), C.c_int64(), C.c_int()
    check(lib.e2vq_wav_info(str(path).encode(), C.byref(sr), C.byref(n), C.byref(bits)))
    return sr.value, n.value, bits.value


def wav_read(path):
    """(samples as int32, sample_rate)."""
    sr, n, _bits = wav_info(path)
    s = np.zeros(n, dtype=np.int32)
    check(lib.e2vq_wav_read(str(path).encode(), s.ctypes.data, n))
    return s, sr


def analyze(samples, sample_rate, P=36, W=45, O=15, device=0, out="numpy"):
    """LPC analysis of one integer signal -> (frames (T, P+1) float64, status (T,) int32).

    Rows whose status is not 0 (the Levinson recursion failed: 1 = r[0] == 0, 2 = prediction error <= 0) are zeros;
    ``ecoz2 lpc`` leaves them out of the .prd.  out="torch": CUDA/HIP tensors on ``device`` (the frames can go to
    ``VqSession.set_frames`` once the failed rows are dropped)."""
    s = np.asarray(samples)
    if s.ndim != 1 or s.dtype.kind not in "iu":
        raise TypeError("samples: a 1-D array of integer PCM values")
    s = np.ascontiguousarray(s, dtype=np.int32)
    T = C.c_int64()
    check(lib.e2vq_lpc_analyze(int(device), int(P), int(W), int(O), s.ctypes.data, len(s), int(sample_rate), None, None,
                               0, C.byref(T), 0))
    T = T.value
    if out == "torch":
        import torch

        dev = torch.device("cuda", device)
        frames = torch.empty((T, P + 1), dtype=torch.float64, device=dev)
        status = torch.empty(T, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        check(lib.e2vq_lpc_analyze(int(device), int(P), int(W), int(O), s.ctypes.data, len(s), int(sample_rate),
                                   frames.data_ptr(), status.data_ptr(), T, C.byref(C.c_int64()), 1))
        return frames, status
    if out != "numpy":
        raise ValueError(f"out: 'numpy' or 'torch', not {out!r}")
    frames = np.zeros((T, P + 1))
    status = np.zeros(T, dtype=np.int32)
    check(lib.e2vq_lpc_analyze(int(device), int(P), int(W), int(O), s.ctypes.data, len(s), int(sample_rate),
                               frames.ctypes.data, status.ctypes.data, T, C.byref(C.c_int64()), 0))
    return frames, status


def lpca(x, p):
    """ecoz2_lpca on one windowed frame (host) -> (status, pe, r, rc, a), as lpca1 (src/lpc/lpca_rs.rs:28-75)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    r, rc, a = (np.zeros(p + 1) for _ in range(3))
    pe = C.c_double()
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    st = lib.ecoz2_lpca(dp(x), len(x), int(p), dp(r), dp(rc), dp(a), C.byref(pe))
    if st < 0:
        check(1)
    return st, pe.value, r, rc, a


def lpca_batch(x, p, device=0):
    """Batched lpca on the GPU: x (count, n) windowed frames -> (status, pe, r, rc, a) arrays."""
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    count, n = x.shape
    r, rc, a = (np.zeros((count, p + 1)) for _ in range(3))
    pe = np.zeros(count)
    st = np.zeros(count, dtype=np.int32)
    check(lib.e2vq_lpca_batch(int(device), int(p), x.ctypes.data, n, count, r.ctypes.data, rc.ctypes.data, a.ctypes.data,
                              pe.ctypes.data, st.ctypes.data))
    return st, pe, r, rc, a


FEATURES = ("status", "pe", "rc", "a", "c")
MAX_Q = 1024  # E2VQ_LPC_FEATURES_MAX_Q


def features(frames, q=0, device=0, want=FEATURES):
    """LPC features of stored vectors r (T, P+1) float64 -> dict of the outputs named in ``want``:
    status (T,) int32, pe (T,), rc and a (T, P+1), c (T, q) (only when q > 0; P < q <= MAX_Q).

    lpca_r (src/lpc/lpca_r_rs.rs) and lpca_get_cepstrum (src/lpc/lpca_cepstrum_rs.rs) of the reference, bit for bit
    (DESIGN.md 8.1).  status 1 (r[0] == 0) rows are zeros; status 2 rows keep what the recursion left; every row gets a
    cepstrum.  A numpy array in gives numpy arrays out (c[0] = the C library's log(sqrt(pe))); a CUDA/HIP torch tensor
    gives tensors on its device, with no host copy (c[0] from the device log, within 1 ulp of the host's)."""
    want = tuple(want)
    if q == 0 and want == FEATURES:  # the default: everything there is
        want = FEATURES[:-1]
    bad = [w for w in want if w not in FEATURES]
    if bad:
        raise ValueError(f"want: names among {FEATURES}, not {bad}")
    if "c" in want and q == 0:
        raise ValueError("want 'c' needs q > 0")
    is_torch = type(frames).__module__.startswith("torch")
    if is_torch:
        import torch

        if not frames.is_cuda or frames.dtype != torch.float64 or frames.dim() != 2:
            raise TypeError("frames: a 2-D torch.float64 tensor on a CUDA/HIP device, or a numpy array")
        fr = frames.contiguous()
        dev = fr.device
        T, NC = fr.shape
        out = {}
        for w in want:
            if w == "status":
                out[w] = torch.empty(T, dtype=torch.int32, device=dev)
            elif w == "pe":
                out[w] = torch.empty(T, dtype=torch.float64, device=dev)
            elif w == "c":
                out[w] = torch.empty((T, q), dtype=torch.float64, device=dev)
            else:
                out[w] = torch.empty((T, NC), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        ptr = lambda w: out[w].data_ptr() if w in out and T > 0 else None  # noqa: E731
        check(lib.e2vq_lpc_features(dev.index if dev.index is not None else int(device), NC - 1, int(q),
                                    fr.data_ptr() if T > 0 else 1, T, ptr("status"), ptr("pe"), ptr("rc"), ptr("a"),
                                    ptr("c"), 1))
        return out
    fr = np.ascontiguousarray(frames, dtype=np.float64)
    if fr.ndim != 2:
        raise TypeError("frames: a (T, P+1) array")
    T, NC = fr.shape
    out = {}
    for w in want:
        if w == "status":
            out[w] = np.zeros(T, dtype=np.int32)
        elif w == "pe":
            out[w] = np.zeros(T)
        elif w == "c":
            out[w] = np.zeros((T, q))
        else:
            out[w] = np.zeros((T, NC))
    ptr = lambda w: out[w].ctypes.data if w in out else None  # noqa: E731
    check(lib.e2vq_lpc_features(int(device), NC - 1, int(q), fr.ctypes.data, T, ptr("status"), ptr("pe"), ptr("rc"),
                                ptr("a"), ptr("c"), 0))
    return out
