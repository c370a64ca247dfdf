"""numpy restatement of the smoothed class posteriors under class-to-class prices (TEST INFRASTRUCTURE):
e2vq_hmm_segment_trans_posteriors and `hmm segment --class-transitions --grammar-posteriors`, DESIGN.md 4.8.13.

hmm_posterior_restatement.py with the one price sw replaced by w[f][k] = math.exp(lt[f][k]) (the C library's exp, as on the
host): forward, the mass that enters class k is m[k] = sum_f CS_f(ah) w[f][k], the sources in class order; backward, class f
receives r[f] = sum_k w[f][k] R[k] with R[k] = sum_j pi_k[j] u[k][j].  Every operation is one IEEE double operation in the
contract's order (numpy forms no fma).  `transcribe` is the contract written out literally in plain Python loops;
`posteriors_one` is the same operations vectorised per run of consecutive classes of one N and sequential in t, along every
chain and along both walks.  The global sum, the packing and the scaling are hmm_posterior_restatement's.
"""
import math

import numpy as np

from .hmm_posterior_restatement import MAX_SLOTS, NINF, _Sum, _result, log_prob, packing, scale_step


def prices(ln_trans, K):
    lt = np.asarray(ln_trans, dtype=np.float64)
    assert lt.shape == (K, K)
    return np.array([[math.exp(float(v)) for v in row] for row in lt], dtype=np.float64).reshape(K, K)


def posteriors_one(models, seq, ln_trans):
    """one stream under the class loop of models = [(pi, A, B)] and the K x K prices -> dict post (T, K), log_prob, status"""
    models = [tuple(np.asarray(x, dtype=np.float64) for x in m) for m in models]
    seq = np.asarray(seq, dtype=np.int64)
    K, T, M = len(models), len(seq), models[0][2].shape[1]
    Ns = [len(m[0]) for m in models]
    w = prices(ln_trans, K)
    if T == 0:
        return _result(0, K, 0)
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

    ahs, cs = [], []
    p, E = 0.5, 1
    ah = None
    for t in range(T):
        o = seq[t]
        if o >= M:
            return _result(T, K, 2)
        if t == 0:
            x = [pi * B[:, :, o] for pi, _A, B in runs]
        else:
            S = class_sums(ah)
            # m[k] over all k at once, the sources f in class order (accumulate adds strictly one after the other)
            m = np.add.accumulate(S[:, None] * w, axis=0)[-1]
            x = []
            for r, ((pi, A, B), a) in enumerate(zip(runs, ah)):
                prod = a[:, :, None] * A  # prod[k, i, j] = ah[k][i] * A_k[i][j]
                acc = prod[:, 0, :].copy()
                for i in range(1, A.shape[1]):
                    np.add(acc, prod[:, i, :], out=acc)
                x.append((acc + m[at[r]:at[r + 1], None] * pi) * B[:, :, o])
        c = GS(flat(x))
        if not c > 0.0:
            return _result(T, K, 1)
        ah = [v / c for v in x]
        ahs.append(ah)
        cs.append(c)
        p, E = scale_step(c, p, E)
    post = np.zeros((T, K))
    bh = [np.ones_like(pi) for pi, _A, _B in runs]
    for t in range(T - 1, -1, -1):
        post[t] = class_sums([a * b for a, b in zip(ahs[t], bh)])
        if t == 0:
            break
        o = seq[t]
        u = [(B[:, :, o] * b) / cs[t] for (_pi, _A, B), b in zip(runs, bh)]
        R = class_sums([pi * v for (pi, _A, _B), v in zip(runs, u)])
        r = np.add.accumulate(w * R[None, :], axis=1)[:, -1]  # r[f] over all f at once, the targets k in class order
        bh = []
        for i, ((_pi, A, _B), v) in enumerate(zip(runs, u)):
            prod = A * v[:, None, :]  # prod[k, i, j] = A_k[i][j] * u[k][j]
            acc = prod[:, :, 0].copy()
            for j in range(1, A.shape[1]):
                np.add(acc, prod[:, :, j], out=acc)
            bh.append(acc + r[at[i]:at[i + 1], None])
    return dict(post=post, log_prob=log_prob(p, E), status=0)


def posteriors(models, sym, offs, ln_trans):
    """the layout of ecoz2rs_amd.hmm.segment_trans_posteriors: post (sum T_s, K), per stream log_prob and status"""
    sym = np.asarray(sym)
    K = len(models)
    outs = [posteriors_one(models, sym[a:b], ln_trans) for a, b in zip(offs[:-1], offs[1:])]
    return dict(post=np.concatenate([o["post"] for o in outs]) if outs else np.zeros((0, K)),
                log_prob=np.array([o["log_prob"] for o in outs], dtype=np.float64),
                status=np.array([o["status"] for o in outs], dtype=np.int32))


def transcribe(models, seq, ln_trans):
    """the contract of DESIGN.md 4.8.13, literally: -> (post as T lists of K floats, ln P(O | loop), status)"""
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
        return [], 0.0, 0
    zero = [[0.0] * K for _ in range(T)]
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
            return zero, NINF, 2
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
                    acc = ah[k][0] * A[k][0][j]
                    for i in range(1, Ns[k]):
                        acc = acc + ah[k][i] * A[k][i][j]
                    xk.append((acc + m * pi[k][j]) * B[k][j][o[t]])
                x.append(xk)
        c = GS(x)
        if not c > 0.0:
            return zero, NINF, 1
        ahs.append([[v / c for v in xk] for xk in x])
        cs.append(c)
        p, E = scale_step(c, p, E)
    post = [None] * T
    bh = [[1.0] * N for N in Ns]
    for t in range(T - 1, -1, -1):
        post[t] = [CS([[ahs[t][k][j] * bh[k][j] for j in range(Ns[k])] for k in range(K)], k) for k in range(K)]
        if t == 0:
            break
        u = [[(B[k][j][o[t]] * bh[k][j]) / cs[t] for j in range(Ns[k])] for k in range(K)]
        R = []
        for k in range(K):
            s = pi[k][0] * u[k][0]
            for j in range(1, Ns[k]):
                s = s + pi[k][j] * u[k][j]
            R.append(s)
        nb = []
        for f in range(K):
            r = w[f][0] * R[0]
            for k in range(1, K):
                r = r + w[f][k] * R[k]
            bk = []
            for i in range(Ns[f]):
                acc = A[f][i][0] * u[f][0]
                for j in range(1, Ns[f]):
                    acc = acc + A[f][i][j] * u[f][j]
                bk.append(acc + r)
            nb.append(bk)
        bh = nb
    return post, log_prob(p, E), 0
