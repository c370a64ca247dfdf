"""numpy restatement of HMM Viterbi decoding (TEST INFRASTRUCTURE): e2vq_hmm_viterbi and `seq show -P / -Q`,
DESIGN.md 4.8.1.

The logarithms are math.log element by element (the C library's log, as the host of the product takes them) with
log 0 = -inf; numpy's own log need not be the C library's.  Every step of the recursion is one IEEE double addition,
vectorised over the states and sequential in t; np.argmax returns the first maximum, which is the contract's strict `>`
with the lowest index winning ties.  `transcribe` is the contract written out literally in plain Python loops.
"""
import math

import numpy as np

NINF = float("-inf")


def logs(x):
    """element-wise math.log, 0 -> -inf (the model is checked to hold finite non-negative values)"""
    x = np.asarray(x, dtype=np.float64)
    return np.array([math.log(v) if v > 0.0 else NINF for v in x.ravel().tolist()]).reshape(x.shape)


def log_model(pi, A, B):
    return logs(pi), logs(A), logs(B)


def viterbi_logs(lpi, lA, lB, seq):
    """-> (path uint16 (T,), ln P*, status) of one sequence under the model's logarithms"""
    seq = np.asarray(seq, dtype=np.int64)
    N, M = lB.shape
    T = len(seq)
    if T == 0:
        return np.zeros(0, dtype=np.uint16), 0.0, 0
    if np.any(seq >= M):
        return np.full(T, 0xFFFF, dtype=np.uint16), NINF, 2
    psi = np.zeros((T, N), dtype=np.int64)
    d = lpi + lB[:, seq[0]]
    cols = np.arange(N)
    for t in range(1, T):
        v = d[:, None] + lA  # v[i, j] = d[i] + lA[i][j]
        arg = np.argmax(v, axis=0)
        d = v[arg, cols] + lB[:, seq[t]]
        psi[t] = arg
    q = np.zeros(T, dtype=np.int64)
    q[T - 1] = int(np.argmax(d))
    lp = float(d[q[T - 1]])
    for t in range(T - 2, -1, -1):
        q[t] = psi[t + 1, q[t + 1]]
    return q.astype(np.uint16), lp, (1 if lp == NINF else 0)


def viterbi(pi, A, B, seqs):
    """-> dict(path=[uint16 arrays], log_prob=(S,), status=(S,)), the layout of ecoz2rs_amd.hmm.viterbi"""
    lpi, lA, lB = log_model(pi, A, B)
    out = [viterbi_logs(lpi, lA, lB, s) for s in seqs]
    return dict(path=[o[0] for o in out], log_prob=np.array([o[1] for o in out], dtype=np.float64),
                status=np.array([o[2] for o in out], dtype=np.int32))


def transcribe(pi, A, B, seq):
    """the contract of DESIGN.md 4.8.1, literally: -> (path list, ln P*, status)"""
    N, M = len(pi), len(B[0])
    lg = lambda x: math.log(x) if x > 0.0 else NINF
    lpi = [lg(float(pi[j])) for j in range(N)]
    lA = [[lg(float(A[i][j])) for j in range(N)] for i in range(N)]
    lB = [[lg(float(B[j][k])) for k in range(M)] for j in range(N)]
    o = [int(x) for x in seq]
    T = len(o)
    if T == 0:
        return [], 0.0, 0
    if any(x >= M for x in o):
        return [0xFFFF] * T, NINF, 2
    d = [lpi[j] + lB[j][o[0]] for j in range(N)]
    psi = [[0] * N]
    for t in range(1, T):
        nd, row = [0.0] * N, [0] * N
        for j in range(N):
            best, arg = d[0] + lA[0][j], 0
            for i in range(1, N):
                v = d[i] + lA[i][j]
                if v > best:
                    best, arg = v, i
            nd[j] = best + lB[j][o[t]]
            row[j] = arg
        d = nd
        psi.append(row)
    best, q = d[0], 0
    for j in range(1, N):
        if d[j] > best:
            best, q = d[j], j
    path = [0] * T
    path[T - 1] = q
    for t in range(T - 2, -1, -1):
        path[t] = psi[t + 1][path[t + 1]]
    return path, best, (1 if best == NINF else 0)


def abbreviated(values, full):
    """the value list of `seq show`'s symbol line: all when full or L <= 30, else the first 10, `...`, the last 10"""
    v = [str(int(x)) for x in values]
    if full or len(v) <= 30:
        return ", ".join(v)
    return ", ".join(v[:10]) + ", ..., " + ", ".join(v[-10:])
