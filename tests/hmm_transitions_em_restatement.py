"""numpy restatement of Baum-Welch for the class-to-class prices (TEST INFRASTRUCTURE): e2vq_hmm_transitions_estep,
e2vq_hmm_train_transitions and `hmm transitions --em`, DESIGN.md 4.8.14.

Forward, scaling, status, ln P and backward are hmm_trans_posterior_restatement's (4.8.13) word for word; what that pass throws
away is kept: for every stream of status 0, t = 1 .. T - 1 and pair (f, k)
    xi_t[f][k] = S_t[f] * (w[f][k] * R_t[k])
with S_t[f] = CS_f(ah_{t-1}) (the mass the forward step used), R_t[k] the backward entry sum and w[f][k] * R_t[k] the term the
backward walk adds into r[f].  Each xi goes through fix2 (hmm_embedded_restatement's) into the int64 limb pair acc[2 (f K + k)],
acc[2 (f K + k) + 1]; acc[2 K^2] counts the status-0 streams, acc[2 K^2 + 1] the others.  `transcribe` is the contract written out
literally in plain Python loops; `estep_one` is the same operations vectorised per run of consecutive classes of one N and
sequential in t.  The M-step and the loop are the host's: math.exp / math.log are the C library's.
"""
import math

import numpy as np

from .hmm_embedded_restatement import ACC_SHIFT, MAX_ESTEPS, fix2, unfix
from .hmm_posterior_restatement import MAX_SLOTS, NINF, _Sum, log_prob, packing, scale_step
from .hmm_trans_posterior_restatement import prices


def acc_words(K):
    return 2 * K * K + 2


def new_acc(K):
    return np.zeros(acc_words(K), dtype=np.int64)


def _count(acc, K, status):
    acc[2 * K * K + (0 if status == 0 else 1)] += 1


def estep_one(models, seq, ln_trans, acc):
    """one stream under the class loop of models = [(pi, A, B)] and the K x K prices: its counts added to acc -> (ln P, status)"""
    models = [tuple(np.asarray(x, dtype=np.float64) for x in m) for m in models]
    seq = np.asarray(seq, dtype=np.int64)
    K, T, M = len(models), len(seq), models[0][2].shape[1]
    Ns = [len(m[0]) for m in models]
    w = prices(ln_trans, K)
    if T == 0:
        _count(acc, K, 0)
        return 0.0, 0
    GS = _Sum(Ns)
    assert GS.slots <= MAX_SLOTS
    runs, at = [], []  # consecutive classes of one N, computed at once: pi (Kb, N), A (Kb, N, N), B (Kb, N, M); first class
    for k, m in enumerate(models):
        if runs and runs[-1][0] == Ns[k]:
            runs[-1][1].append(m)
        else:
            runs.append((Ns[k], [m]))
            at.append(k)
    runs = [tuple(np.stack([m[i] for m in ms]) for i in range(3)) for _N, ms in runs]
    at.append(K)
    flat = lambda xs: np.concatenate([x.ravel() for x in xs])

    def class_sums(vs):  # CS_k of every class: state order
        out = []
        for v in vs:
            s = v[:, 0].copy()
            for j in range(1, v.shape[1]):
                np.add(s, v[:, j], out=s)
            out.append(s)
        return np.concatenate(out)

    Ss, cs = [None], []  # Ss[t]: S_t, the masses the forward step of frame t used
    p, E = 0.5, 1
    ah = None
    for t in range(T):
        o = seq[t]
        if o >= M:
            _count(acc, K, 2)
            return NINF, 2
        if t == 0:
            x = [pi * B[:, :, o] for pi, _A, B in runs]
        else:
            S = class_sums(ah)
            Ss.append(S)
            # m[k] over all k at once, the sources f in class order (accumulate adds strictly one after the other)
            m = np.add.accumulate(S[:, None] * w, axis=0)[-1]
            x = []
            for r, ((pi, A, B), a) in enumerate(zip(runs, ah)):
                prod = a[:, :, None] * A  # prod[k, i, j] = ah[k][i] * A_k[i][j]
                a_acc = prod[:, 0, :].copy()
                for i in range(1, A.shape[1]):
                    np.add(a_acc, prod[:, i, :], out=a_acc)
                x.append((a_acc + m[at[r]:at[r + 1], None] * pi) * B[:, :, o])
        c = GS(flat(x))
        if not c > 0.0:
            _count(acc, K, 1)
            return NINF, 1
        ah = [v / c for v in x]
        cs.append(c)
        p, E = scale_step(c, p, E)
    _count(acc, K, 0)
    hi_sum = np.zeros((K, K), dtype=np.int64)
    lo_sum = np.zeros((K, K), dtype=np.int64)
    bh = [np.ones_like(pi) for pi, _A, _B in runs]
    for t in range(T - 1, 0, -1):
        o = seq[t]
        u = [(B[:, :, o] * b) / cs[t] for (_pi, _A, B), b in zip(runs, bh)]
        R = class_sums([pi * v for (pi, _A, _B), v in zip(runs, u)])
        wR = w * R[None, :]  # the terms of the walk: wR[f][k] = w[f][k] * R[k]
        r = np.add.accumulate(wR, axis=1)[:, -1]  # r[f] over all f at once, the targets k in class order
        hi, lo = fix2(Ss[t][:, None] * wR)
        hi_sum += hi
        lo_sum += lo
        bh = []
        for i, ((_pi, A, _B), v) in enumerate(zip(runs, u)):
            prod = A * v[:, None, :]  # prod[k, i, j] = A_k[i][j] * u[k][j]
            b_acc = prod[:, :, 0].copy()
            for j in range(1, A.shape[1]):
                np.add(b_acc, prod[:, :, j], out=b_acc)
            bh.append(b_acc + r[at[i]:at[i + 1], None])
    acc[0:2 * K * K:2] += hi_sum.ravel()
    acc[1:2 * K * K:2] += lo_sum.ravel()
    return log_prob(p, E), 0


def estep(models, sym, offs, ln_trans, acc=None, one=estep_one):
    """the layout of ecoz2rs_amd.hmm.transitions_estep: acc (2 K^2 + 2 int64, added to where given), per stream log_prob, status"""
    sym = np.asarray(sym)
    K = len(models)
    acc = new_acc(K) if acc is None else acc
    lps, sts = [], []
    for a, b in zip(offs[:-1], offs[1:]):
        lp, st = one(models, sym[a:b], ln_trans, acc)
        lps.append(lp)
        sts.append(st)
    return dict(acc=acc, log_prob=np.array(lps, dtype=np.float64), status=np.array(sts, dtype=np.int32))


def counts(acc, K):
    """acc -> the expected counts C (K, K) as floats, each cell unfixed once"""
    return np.array([[unfix(acc[2 * (f * K + k)], acc[2 * (f * K + k) + 1]) for k in range(K)] for f in range(K)])


def row_mass(acc, K, f):
    """D[f]: the integer sum of row f, both limbs, unfixed once"""
    hi = sum(int(acc[2 * (f * K + k)]) for k in range(K))
    lo = sum(int(acc[2 * (f * K + k) + 1]) for k in range(K))
    return unfix(hi, lo)


def mstep(ln_p, acc, alpha):
    """the M-step of the contract -> the new matrix as the file holds it"""
    ln_p = np.array(ln_p, dtype=np.float64)
    K = ln_p.shape[0]
    for f in range(K):
        n = sum(1 for k in range(K) if ln_p[f, k] != NINF)
        den = row_mass(acc, K, f) + alpha * float(n)
        if not den > 0.0:
            continue
        for k in range(K):
            if ln_p[f, k] != NINF:
                P = (unfix(acc[2 * (f * K + k)], acc[2 * (f * K + k) + 1]) + alpha) / den
                ln_p[f, k] = math.log(P) if P > 0.0 else NINF
    return ln_p


def train(models, sym, offs, ln_p=None, ln_switch=0.0, alpha=1.0, val_auto=0.3, max_iterations=-1, one=estep_one):
    """the loop of the contract -> (ln_p, [sum ln P per E-step]); raises ValueError where the call returns 1"""
    K = len(models)
    ln_p = np.full((K, K), math.log(1.0 / K)) if ln_p is None else np.array(ln_p, dtype=np.float64)
    hist, Lprev, it = [], 0.0, 0
    while True:
        if (max_iterations >= 0 and it >= max_iterations) or it >= MAX_ESTEPS:
            break
        r = estep(models, sym, offs, ln_p + ln_switch, one=one)
        L = 0.0
        for lp, st in zip(r["log_prob"], r["status"]):
            if st == 0:
                L = L + float(lp)
        if it == 0 and not (r["status"] == 0).any():
            raise ValueError("no stream can be explained by the class loop")
        hist.append(L)
        if it > 0 and L - Lprev <= val_auto:
            break
        ln_p = mstep(ln_p, r["acc"], alpha)
        Lprev = L
        it += 1
    return ln_p, hist


def transcribe(models, seq, ln_trans, acc):
    """the contract of DESIGN.md 4.8.14, literally: the stream's counts added to acc -> (ln P(O | loop), status)"""
    K = len(models)
    Ns = [len(m[0]) for m in models]
    M = len(models[0][2][0])
    pi = [[float(m[0][j]) for j in range(N)] for m, N in zip(models, Ns)]
    A = [[[float(m[1][i][j]) for j in range(N)] for i in range(N)] for m, N in zip(models, Ns)]
    B = [[[float(m[2][j][o]) for o in range(M)] for j in range(N)] for m, N in zip(models, Ns)]
    w = [[math.exp(float(ln_trans[f][k])) for k in range(K)] for f in range(K)]
    o = [int(x) for x in seq]
    T = len(o)
    if T == 0:
        _count(acc, K, 0)
        return 0.0, 0
    slot, lane, slots = packing(Ns)
    comp0 = [sum(Ns[:k]) for k in range(K)]

    def GS(x):
        v = [[0.0] * 64 for _ in range(slots)]
        for k in range(K):
            for j in range(Ns[k]):
                v[slot[comp0[k] + j]][lane[comp0[k] + j]] = x[k][j]
        for m in (32, 16, 8, 4, 2, 1):
            v = [[row[l] + row[l ^ m] for l in range(64)] for row in v]
        total = v[0][0]
        for s in range(1, slots):
            total = total + v[s][0]
        return total

    def CS(v, k):
        s = v[k][0]
        for j in range(1, Ns[k]):
            s = s + v[k][j]
        return s

    ahs, cs = [], []
    p, E = 0.5, 1
    for t in range(T):
        if o[t] >= M:
            _count(acc, K, 2)
            return NINF, 2
        if t == 0:
            x = [[pi[k][j] * B[k][j][o[0]] for j in range(Ns[k])] for k in range(K)]
        else:
            ah = ahs[-1]
            S = [CS(ah, f) for f in range(K)]
            x = []
            for k in range(K):
                m = S[0] * w[0][k]
                for f in range(1, K):
                    m = m + S[f] * w[f][k]
                xk = []
                for j in range(Ns[k]):
                    a = ah[k][0] * A[k][0][j]
                    for i in range(1, Ns[k]):
                        a = a + ah[k][i] * A[k][i][j]
                    xk.append((a + m * pi[k][j]) * B[k][j][o[t]])
                x.append(xk)
        c = GS(x)
        if not c > 0.0:
            _count(acc, K, 1)
            return NINF, 1
        ahs.append([[v / c for v in xk] for xk in x])
        cs.append(c)
        p, E = scale_step(c, p, E)
    _count(acc, K, 0)
    bh = [[1.0] * N for N in Ns]
    for t in range(T - 1, 0, -1):
        u = [[(B[k][j][o[t]] * bh[k][j]) / cs[t] for j in range(Ns[k])] for k in range(K)]
        R = []
        for k in range(K):
            s = pi[k][0] * u[k][0]
            for j in range(1, Ns[k]):
                s = s + pi[k][j] * u[k][j]
            R.append(s)
        S = [CS(ahs[t - 1], f) for f in range(K)]
        nb = []
        for f in range(K):
            r = w[f][0] * R[0]
            for k in range(1, K):
                r = r + w[f][k] * R[k]
            for k in range(K):
                hi, lo = fix2(S[f] * (w[f][k] * R[k]))
                acc[2 * (f * K + k)] += int(hi)
                acc[2 * (f * K + k) + 1] += int(lo)
            bk = []
            for i in range(Ns[f]):
                a = A[f][i][0] * u[f][0]
                for j in range(1, Ns[f]):
                    a = a + A[f][i][j] * u[f][j]
                bk.append(a + r)
            nb.append(bk)
        bh = nb
    return log_prob(p, E), 0


__all__ = ["ACC_SHIFT", "acc_words", "counts", "estep", "estep_one", "fix2", "mstep", "new_acc", "row_mass", "train", "transcribe", "unfix"]
