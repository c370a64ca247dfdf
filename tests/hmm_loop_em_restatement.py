"""numpy restatement of Baum-Welch for the class models under the class loop (TEST INFRASTRUCTURE): e2vq_hmm_loop_estep,
e2vq_hmm_train_loop and `hmm learn --loop`, DESIGN.md 4.8.16.

Forward, scaling, status, ln P and backward are hmm_trans_posterior_restatement's (4.8.13) word for word; new are the state
counts of every stream of status 0, each through fix2 (hmm_embedded_restatement's) into class k's block in the layout of
hmm_embedded_restatement.layout (PI | AN | AD | BN | BD | used, skipped):
    every t:     g = ah_t[k][j] * bh_t[k][j]                    -> BN[j][o_t], BD[j]; at t = 0 also PI[j]
    t < T - 1:   (ah_t[k][i] * A_k[i][j]) * u_{t+1}[k][j]       -> AN[i][j]
    t < T - 1:   (m_{t+1}[k] * pi_k[j]) * u_{t+1}[k][j]         -> PI[j]
with u_{t+1} = (B_k[j][o_{t+1}] * bh_{t+1}[k][j]) / c_{t+1} and m the mass the forward step added through pi.  AD is the
integer row sum of AN; used / skipped count the streams in every class's block.  With acc_t the grammar counts of
hmm_transitions_em_restatement (4.8.14) are added to it, limb for limb that restatement's.  `transcribe` is the contract written
out literally in plain Python loops; `estep_one` is the same operations vectorised per run of consecutive classes of one N and
sequential in t.  The M-steps and the loop are the host's and the sibling restatements': hmm_embedded_restatement.mstep for the
models, hmm_transitions_em_restatement.mstep for the matrix.
"""
import math

import numpy as np

from . import hmm_embedded_restatement as R11
from . import hmm_transitions_em_restatement as R14
from .hmm_embedded_restatement import ACC_SHIFT, MAX_ESTEPS, acc_words, decode, fix2, layout, unfix
from .hmm_posterior_restatement import MAX_SLOTS, NINF, _Sum, log_prob, packing, scale_step
from .hmm_trans_posterior_restatement import prices


def new_accs(models):
    M = np.asarray(models[0][2]).shape[1]
    return [np.zeros(acc_words(len(m[0]), M), dtype=np.int64) for m in models]


def _mark(accs, models, status, acc_t):
    """the stream's mark: in every class's block (every class is in the loop), and in the grammar table where one is given"""
    M = np.asarray(models[0][2]).shape[1]
    for k, acc in enumerate(accs):
        acc[layout(len(models[k][0]), M)["used" if status == 0 else "skipped"]] += 1
    if acc_t is not None:
        R14._count(acc_t, len(models), status)


def rowsums(accs, models):
    R11._rowsums(accs, models)


def estep_one(models, seq, ln_trans, accs, acc_t=None):
    """one stream under the class loop of models = [(pi, A, B)] and the K x K prices: its counts added to accs (AD is left to
    rowsums) and, where given, to acc_t -> (ln P, status)"""
    models = [tuple(np.asarray(x, dtype=np.float64) for x in m) for m in models]
    seq = np.asarray(seq, dtype=np.int64)
    K, T, M = len(models), len(seq), models[0][2].shape[1]
    Ns = [len(m[0]) for m in models]
    w = prices(ln_trans, K)
    if T == 0:
        _mark(accs, models, 0, acc_t)
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

    ahs, Ss, ms, cs = [], [None], [None], []  # Ss[t], ms[t]: what the forward step of frame t used
    p, E = 0.5, 1
    ah = None
    for t in range(T):
        o = seq[t]
        if o >= M:
            _mark(accs, models, 2, acc_t)
            return NINF, 2
        if t == 0:
            x = [pi * B[:, :, o] for pi, _A, B in runs]
        else:
            S = class_sums(ah)
            Ss.append(S)
            # m[k] over all k at once, the sources f in class order (accumulate adds strictly one after the other)
            m = np.add.accumulate(S[:, None] * w, axis=0)[-1]
            ms.append(m)
            x = []
            for r, ((pi, A, B), a) in enumerate(zip(runs, ah)):
                prod = a[:, :, None] * A  # prod[k, i, j] = ah[k][i] * A_k[i][j]
                a_acc = prod[:, 0, :].copy()
                for i in range(1, A.shape[1]):
                    np.add(a_acc, prod[:, i, :], out=a_acc)
                x.append((a_acc + m[at[r]:at[r + 1], None] * pi) * B[:, :, o])
        c = GS(flat(x))
        if not c > 0.0:
            _mark(accs, models, 1, acc_t)
            return NINF, 1
        ah = [v / c for v in x]
        ahs.append(ah)
        cs.append(c)
        p, E = scale_step(c, p, E)
    _mark(accs, models, 0, acc_t)

    class Limbs:  # hi and lo of the cells of one kind of one run
        def __init__(self, shape):
            self.hi, self.lo = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)

        def add(self, val, at=None):
            hi, lo = fix2(val)
            if at is None:
                self.hi += hi
                self.lo += lo
            else:
                self.hi[at] += hi
                self.lo[at] += lo

    tabs = [dict(PI=Limbs(pi.shape), AN=Limbs(A.shape), BN=Limbs(B.shape), BD=Limbs(pi.shape)) for pi, A, B in runs]
    c_hi = np.zeros((K, K), dtype=np.int64)
    c_lo = np.zeros((K, K), dtype=np.int64)
    bh = [np.ones_like(pi) for pi, _A, _B in runs]
    for t in range(T - 1, -1, -1):
        o = seq[t]
        for tab, a, b in zip(tabs, ahs[t], bh):
            g = a * b
            tab["BN"].add(g, (slice(None), slice(None), o))
            tab["BD"].add(g)
            if t == 0:
                tab["PI"].add(g)
        if t == 0:
            break
        u = [(B[:, :, o] * b) / cs[t] for (_pi, _A, B), b in zip(runs, bh)]
        R = class_sums([pi * v for (pi, _A, _B), v in zip(runs, u)])
        wR = w * R[None, :]  # the terms of the walk: wR[f][k] = w[f][k] * R[k]
        r = np.add.accumulate(wR, axis=1)[:, -1]  # r[f] over all f at once, the targets k in class order
        if acc_t is not None:
            hi, lo = fix2(Ss[t][:, None] * wR)
            c_hi += hi
            c_lo += lo
        nb = []
        for i, ((pi, A, _B), v, ap, tab) in enumerate(zip(runs, u, ahs[t - 1], tabs)):
            tab["PI"].add((ms[t][at[i]:at[i + 1], None] * pi) * v)
            tab["AN"].add((ap[:, :, None] * A) * v[:, None, :])
            prod = A * v[:, None, :]  # prod[k, i, j] = A_k[i][j] * u[k][j]
            b_acc = prod[:, :, 0].copy()
            for j in range(1, A.shape[1]):
                np.add(b_acc, prod[:, :, j], out=b_acc)
            nb.append(b_acc + r[at[i]:at[i + 1], None])
        bh = nb
    for i, tab in enumerate(tabs):
        for q, k in enumerate(range(at[i], at[i + 1])):
            lay = layout(Ns[k], M)
            for name in ("PI", "AN", "BN", "BD"):
                n = tab[name].hi[q].size
                accs[k][lay[name]:lay[name] + 2 * n:2] += tab[name].hi[q].ravel()
                accs[k][lay[name] + 1:lay[name] + 2 * n:2] += tab[name].lo[q].ravel()
    if acc_t is not None:
        acc_t[0:2 * K * K:2] += c_hi.ravel()
        acc_t[1:2 * K * K:2] += c_lo.ravel()
    return log_prob(p, E), 0


def estep(models, sym, offs, ln_trans, acc_trans=None, one=estep_one):
    """the layout of ecoz2rs_amd.hmm.loop_estep: acc (per class its words, from zero), per stream log_prob and status; acc_trans:
    None, True (a new table) or a table of hmm_transitions_em_restatement.acc_words(K) words to add into -> also acc_trans"""
    sym = np.asarray(sym)
    accs = new_accs(models)
    if acc_trans is True:
        acc_trans = R14.new_acc(len(models))
    lps, sts = [], []
    for a, b in zip(offs[:-1], offs[1:]):
        lp, st = one(models, sym[a:b], ln_trans, accs, acc_trans)
        lps.append(lp)
        sts.append(st)
    rowsums(accs, models)
    out = dict(acc=accs, log_prob=np.array(lps, dtype=np.float64), status=np.array(sts, dtype=np.int32))
    if acc_trans is not None:
        out["acc_trans"] = acc_trans
    return out


def mstep(models, accs, epsilon, frozen=None):
    """the M-step of the models: the block of a frozen class is zeroed first, then 4.8.11's M-step -> new models"""
    accs = [np.zeros_like(a) if frozen is not None and frozen[k] else a for k, a in enumerate(accs)]
    return R11.mstep(models, accs, epsilon)


def train(models, sym, offs, ln_p=None, ln_switch=0.0, train_transitions=False, frozen=None, alpha=1.0, epsilon=1e-5, val_auto=0.3,
          max_iterations=-1, one=estep_one):
    """the loop of the contract -> (models, ln_p, [sum ln P per E-step]); raises ValueError where the call returns 1"""
    K = len(models)
    models = [tuple(np.array(x, dtype=np.float64) for x in m) for m in models]
    ln_p = np.zeros((K, K)) if ln_p is None else np.array(ln_p, dtype=np.float64)
    hist, Lprev, it = [], 0.0, 0
    while True:
        if (max_iterations >= 0 and it >= max_iterations) or it >= MAX_ESTEPS:
            break
        r = estep(models, sym, offs, ln_p + ln_switch, acc_trans=True if train_transitions else None, one=one)
        L = 0.0
        for lp, st in zip(r["log_prob"], r["status"]):
            if st == 0:
                L = L + float(lp)
        if it == 0 and not (r["status"] == 0).any():
            raise ValueError("no stream can be explained by the class loop")
        hist.append(L)
        if it > 0 and L - Lprev <= val_auto:
            break
        models = mstep(models, r["acc"], epsilon, frozen)
        if train_transitions:
            ln_p = R14.mstep(ln_p, r["acc_trans"], alpha)
        Lprev = L
        it += 1
    return models, ln_p, hist


def transcribe(models, seq, ln_trans, accs, acc_t=None):
    """the contract of DESIGN.md 4.8.16, literally: the stream's counts added to accs (and acc_t) -> (ln P(O | loop), status)"""
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
        _mark(accs, models, 0, acc_t)
        return 0.0, 0
    slot, lane, slots = packing(Ns)
    comp0 = [sum(Ns[:k]) for k in range(K)]
    lays = [layout(N, M) for N in Ns]

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

    def add(k, name, cell, x):
        hi, lo = fix2(x)
        accs[k][lays[k][name] + 2 * cell] += int(hi)
        accs[k][lays[k][name] + 2 * cell + 1] += int(lo)

    ahs, ms, cs = [], [None], []
    p, E = 0.5, 1
    for t in range(T):
        if o[t] >= M:
            _mark(accs, models, 2, acc_t)
            return NINF, 2
        if t == 0:
            x = [[pi[k][j] * B[k][j][o[0]] for j in range(Ns[k])] for k in range(K)]
        else:
            ah = ahs[-1]
            S = [CS(ah, f) for f in range(K)]
            x, mt = [], []
            for k in range(K):
                m = S[0] * w[0][k]
                for f in range(1, K):
                    m = m + S[f] * w[f][k]
                mt.append(m)
                xk = []
                for j in range(Ns[k]):
                    a = ah[k][0] * A[k][0][j]
                    for i in range(1, Ns[k]):
                        a = a + ah[k][i] * A[k][i][j]
                    xk.append((a + m * pi[k][j]) * B[k][j][o[t]])
                x.append(xk)
            ms.append(mt)
        c = GS(x)
        if not c > 0.0:
            _mark(accs, models, 1, acc_t)
            return NINF, 1
        ahs.append([[v / c for v in xk] for xk in x])
        cs.append(c)
        p, E = scale_step(c, p, E)
    _mark(accs, models, 0, acc_t)
    bh = [[1.0] * N for N in Ns]
    for t in range(T - 1, -1, -1):
        for k in range(K):
            for j in range(Ns[k]):
                g = ahs[t][k][j] * bh[k][j]
                add(k, "BN", j * M + o[t], g)
                add(k, "BD", j, g)
                if t == 0:
                    add(k, "PI", j, g)
        if t == 0:
            break
        u = [[(B[k][j][o[t]] * bh[k][j]) / cs[t] for j in range(Ns[k])] for k in range(K)]
        for k in range(K):
            for j in range(Ns[k]):
                add(k, "PI", j, (ms[t][k] * pi[k][j]) * u[k][j])
                for i in range(Ns[k]):
                    add(k, "AN", i * Ns[k] + j, (ahs[t - 1][k][i] * A[k][i][j]) * u[k][j])
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
            if acc_t is not None:
                for k in range(K):
                    hi, lo = fix2(S[f] * (w[f][k] * R[k]))
                    acc_t[2 * (f * K + k)] += int(hi)
                    acc_t[2 * (f * K + k) + 1] += int(lo)
            bk = []
            for i in range(Ns[f]):
                a = A[f][i][0] * u[f][0]
                for j in range(1, Ns[f]):
                    a = a + A[f][i][j] * u[f][j]
                bk.append(a + r)
            nb.append(bk)
        bh = nb
    return log_prob(p, E), 0


__all__ = ["ACC_SHIFT", "acc_words", "decode", "estep", "estep_one", "fix2", "layout", "mstep", "new_accs", "rowsums", "train",
           "transcribe", "unfix"]
