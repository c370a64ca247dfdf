"""Extended-precision restatement of the HMM forward-backward (TEST INFRASTRUCTURE): ln P(O) and the Baum-Welch
expected counts of oracle/hmm_oracle.h, computed independently of the oracle's arithmetic.

The oracle and the kernels share one algorithm (scaled forward-backward in f64, frexp bookkeeping of P(O), fix2 limbs
for the counts).  This module shares none of it: every quantity is an np.longdouble (64-bit mantissa on x86-64, eleven
bits more than f64), the forward and backward passes are scaled by their sums but ln P(O) is the sum of the logarithms
of those sums, and the counts are plain sums -- no limbs, no rounding to a fixed grid.  The sums over states run in
numpy's order, not the oracle's chains.

Status codes are the oracle's E-step ones (e2h_accumulate): 0 used, 1 the model cannot emit the sequence or T = 0,
2 some symbol >= M, checked step by step in the oracle's order (a symbol >= M after an impossible step is status 1).
"""
from fractions import Fraction

import numpy as np

LD = np.longdouble
ACC_SHIFT = 29


def require_extended():
    """fail loudly on a host whose long double is no wider than a double"""
    assert np.finfo(LD).nmant >= 63, f"np.longdouble has {np.finfo(LD).nmant} mantissa bits here; this reference needs 63+"


def decode(hi, lo):
    """one accumulator cell (hi, lo) -> its exact value as a Fraction: (hi * 2^31 + lo) * 2^-(29 + 31)"""
    return Fraction(int(hi) * (1 << 31) + int(lo), 1 << (ACC_SHIFT + 31))


def decode_words(acc, N, M):
    """accumulator words (oracle / GPU layout) -> dict of float arrays PI (N,), AN (N, N), AD (N,), BN (N, M), BD (N,)
    and the integer used / skipped counts.  Each value is the exact Fraction rounded once to the nearest double."""
    acc = np.asarray(acc, dtype=np.int64)
    vals = [float(decode(acc[2 * c], acc[2 * c + 1])) for c in range((len(acc) - 2) // 2)]
    v = np.array(vals, dtype=np.float64)
    o = 0
    out = {}
    for name, shape in (("PI", (N,)), ("AN", (N, N)), ("AD", (N,)), ("BN", (N, M)), ("BD", (N,))):
        n = int(np.prod(shape))
        out[name] = v[o:o + n].reshape(shape)
        o += n
    out["used"], out["skipped"] = int(acc[-2]), int(acc[-1])
    return out


def _model(pi, A, B):
    return np.asarray(pi, dtype=LD), np.asarray(A, dtype=LD), np.asarray(B, dtype=LD)


def _forward(pi, A, B, seq):
    """-> (status, alpha_hat (T, N), c (T,)) in long double; status as e2h_forward (T = 0 is status 0 here)"""
    N, M = B.shape
    T = len(seq)
    ah = np.zeros((T, N), dtype=LD)
    c = np.zeros(T, dtype=LD)
    a = None
    for t in range(T):
        o = int(seq[t])
        if o >= M:
            return 2, ah, c
        nx = pi * B[:, o] if t == 0 else (a @ A) * B[:, o]
        s = nx.sum()
        if not s > 0:
            return 1, ah, c
        a = nx / s
        ah[t], c[t] = a, s
    return 0, ah, c


def log_prob(pi, A, B, seq):
    """-> (status, ln P(O)) with the oracle's scoring meanings (T = 0: status 0, ln P = 0)"""
    require_extended()
    pi, A, B = _model(pi, A, B)
    st, _ah, c = _forward(pi, A, B, np.asarray(seq, dtype=np.int64))
    return st, (np.log(c).sum() if st == 0 else LD("-inf"))


def estep(pi, A, B, seqs):
    """-> (status (S,), ln P (S,) as long double, counts dict PI / AN / AD / BN / BD (long double), used, skipped)"""
    require_extended()
    pi, A, B = _model(pi, A, B)
    N, M = B.shape
    PI, AN, AD, BN, BD = (np.zeros(s, dtype=LD) for s in ((N,), (N, N), (N,), (N, M), (N,)))
    status, lps = [], []
    for seq in seqs:
        seq = np.asarray(seq, dtype=np.int64)
        T = len(seq)
        st, ah, c = _forward(pi, A, B, seq) if T else (1, None, None)
        status.append(st)
        lps.append(np.log(c).sum() if st == 0 else LD("-inf"))
        if st != 0:
            continue
        # backward: beta_hat_t = A u_{t+1}, u_{t+1}(j) = B_j(o_{t+1}) beta_hat_{t+1}(j) / c_{t+1}; beta_hat_{T-1} = 1
        beta = np.ones((T, N), dtype=LD)
        u = np.zeros((T, N), dtype=LD)  # u[t] is u_t, used for the step t-1 -> t (u[0] unused)
        for t in range(T - 2, -1, -1):
            u[t + 1] = B[:, seq[t + 1]] * beta[t + 1] / c[t + 1]
            beta[t] = A @ u[t + 1]
        g = ah * beta  # gamma_t(i)
        PI += g[0]
        AD += g[:-1].sum(axis=0)
        BD += g.sum(axis=0)
        np.add.at(BN.T, seq, g)
        if T > 1:  # sum_t xi_t(i, j) = A_ij * sum_t alpha_hat_t(i) u_{t+1}(j)
            AN += A * (ah[:-1].T @ u[1:])
    used = sum(1 for s in status if s == 0)
    counts = dict(PI=PI, AN=AN, AD=AD, BN=BN, BD=BD)
    return np.array(status, dtype=np.int32), np.array(lps, dtype=LD), counts, used, len(seqs) - used
