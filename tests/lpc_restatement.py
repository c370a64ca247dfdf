"""numpy restatement of the reference's Rust LPC analysis (TEST INFRASTRUCTURE).

One signal -> gain-normalised autocorrelation frames, in the operation order of /root/reference/src/lpc/lpc_rs.rs:104-160,
203-250 and lpca_rs.rs:28-75: every step is an element-wise IEEE double operation (numpy never fuses a multiply and an
add), vectorised across frames (and lags), sequential in the sample index -- so each frame's sums are the sequential sums
of the Rust loops.  The Hamming table comes from math.cos, the C library's cos.
"""
import math

import numpy as np


def geometry(N, sample_rate, W, O):
    """(win, off, T) of lpc_rs.rs:203-218; T = -1 when the signal is shorter than one window."""
    win, off = W * sample_rate // 1000, O * sample_rate // 1000
    if off == 0:
        raise ValueError("offset of zero samples")
    if win > N:
        return win, off, -1
    T = (N - (win - off)) // off
    if (T - 1) * off + win > N:
        T -= 1
    return win, off, T


def hamming(win):
    return np.array([0.54 - 0.46 * math.cos(((n * 2) * math.pi) / (win - 1)) for n in range(win)])


def windowed_frames(samples, sample_rate, W, O):
    """(T, win) frames after mean removal, pre-emphasis and the Hamming window (lpc_rs.rs:104-160)."""
    s = np.asarray(samples, dtype=np.float64)  # integer PCM -> f64 is exact
    win, off, T = geometry(len(s), sample_rate, W, O)
    if T < 0:
        raise ValueError("signal too short")
    X = s[np.arange(T)[:, None] * off + np.arange(win)[None, :]]
    acc = np.zeros(T)
    for n in range(win):  # sequential sum left to right
        acc = acc + X[:, n]
    x = X - (acc / win)[:, None]
    y = x.copy()
    y[:, 1:] = x[:, 1:] - 0.95 * x[:, :-1]  # x[n] -= 0.95 * x[n-1], n from win-1 down to 1 (x[n-1] not yet changed)
    return y * hamming(win)[None, :]


def autocorrelation(w, P):
    """r[:, i] = sum_{k=0}^{n-1-i} w[:, k] w[:, k+i], sequential in k (lpca_rs.rs:31-38)."""
    T, n = w.shape
    r = np.zeros((T, P + 1))
    for k in range(n):
        L = min(P + 1, n - k)
        r[:, :L] = r[:, :L] + w[:, k:k + 1] * w[:, k:k + L]
    return r


def levinson(r):
    """lpca_rs.rs:40-72 across frames -> (status, pe); status 0 / 1 (r0 == 0) / 2 (pe <= 0)."""
    T, NC = r.shape
    status = np.where(r[:, 0] == 0.0, 1, 0).astype(np.int32)
    pe = r[:, 0].copy()
    a = np.zeros((T, NC))
    a[:, 0] = 1.0
    with np.errstate(all="ignore"):
        for k in range(1, NC):
            s = np.zeros(T)
            for i in range(1, k + 1):
                s = s - a[:, k - i] * r[:, i]
            akk = s / pe
            a[:, k] = akk
            for i in range(1, (k >> 1) + 1):
                ai, aj = a[:, i].copy(), a[:, k - i].copy()
                a[:, i] = ai + akk * aj
                a[:, k - i] = aj + akk * ai
            pe = pe * (1.0 - akk * akk)
            status[(status == 0) & (pe <= 0.0)] = 2
    return status, pe


def lpca(w, P):
    """lpca1 (lpca_rs.rs:28-75) on windowed frames w (T, n) -> (status, pe, r, rc, a) as lpca1 leaves them: a row stops
    at the step where pe <= 0 first holds (status 2): pe is that non-positive value, rc and a are what the step left,
    zeros beyond it.  A row with r[0] == 0 (status 1) has pe = 0 and rc, a all zero: the kernels' convention
    (lpc_levinson.h); host ecoz2_lpca returns before it writes rc and a there.  rc[0] = 0."""
    r = autocorrelation(np.asarray(w, dtype=np.float64), P)
    T, NC = r.shape
    status = np.where(r[:, 0] == 0.0, 1, 0).astype(np.int32)
    run = status == 0
    pe = np.where(run, r[:, 0], 0.0)
    rc = np.zeros((T, NC))
    a = np.zeros((T, NC))
    a[run, 0] = 1.0
    with np.errstate(all="ignore"):
        for k in range(1, NC):
            s = np.zeros(T)
            for i in range(1, k + 1):
                s = s - a[:, k - i] * r[:, i]
            akk = s / pe
            rc[run, k] = akk[run]
            a[run, k] = akk[run]
            for i in range(1, (k >> 1) + 1):
                ai, aj = a[:, i].copy(), a[:, k - i].copy()
                a[run, i] = (ai + akk * aj)[run]
                a[run, k - i] = (aj + akk * ai)[run]
            pe = np.where(run, pe * (1.0 - akk * akk), pe)
            failed = run & (pe <= 0.0)
            status[failed] = 2
            run = run & ~failed
    return status, pe, r, rc, a


def analyze(samples, sample_rate, P=36, W=45, O=15):
    """-> (frames (T, P+1), status (T,)): r / pe for status 0 (lpc_rs.rs:126-131), zero rows otherwise."""
    r = autocorrelation(windowed_frames(samples, sample_rate, W, O), P)
    status, pe = levinson(r)
    ok = status == 0
    frames = np.zeros_like(r)
    frames[ok] = r[ok] / pe[ok][:, None]
    return frames, status
