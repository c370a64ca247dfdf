"""numpy restatement of the smoothed class posteriors under the class loop (TEST INFRASTRUCTURE): e2vq_hmm_segment_posteriors
and `hmm segment --posteriors`, DESIGN.md 4.8.7.

The arithmetic is linear and scaled; every operation is one IEEE double operation in the contract's order (numpy forms no
fma).  sw = math.exp(ln_switch) is the C library's exp, as on the host.  `transcribe` is the contract written out literally
in plain Python loops; `posteriors_one` is the same operations vectorised per run of consecutive classes of one N and
sequential in t and along every chain.  The global sum depends on the packing of the classes into wave-slots of 64 lanes
(`packing`): per slot a butterfly over the 64 lanes with idle lanes at 0.0, then the slots in order.
"""
import math

import numpy as np

NINF = float("-inf")
MAX_SLOTS = 16


def packing(Ns):
    """class after class; a class that does not fit the open slot of 64 lanes opens the next -> (slot, lane) of every
    composite state, and the number of slots"""
    slot, lane = [], []
    s, fill = -1, 64
    for N in Ns:
        if fill + N > 64:
            s, fill = s + 1, 0
        slot += [s] * N
        lane += list(range(fill, fill + N))
        fill += N
    return np.array(slot, dtype=np.int64), np.array(lane, dtype=np.int64), s + 1


def scale_step(c, p, E):
    m, e = math.frexp(c)
    p, e2 = math.frexp(p * m)
    return p, E + e + e2


def log_prob(p, E):
    return math.log(p) + float(E) * math.log(2.0) if p > 0.0 else NINF


def _result(T, K, status):
    return dict(post=np.zeros((T, K)), log_prob=0.0 if status == 0 else NINF, status=status)


class _Sum:
    """GS of the contract for one packing"""

    def __init__(self, Ns):
        self.slot, self.lane, self.slots = packing(Ns)
        self.perms = [np.arange(64) ^ m for m in (32, 16, 8, 4, 2, 1)]

    def __call__(self, flat):
        v = np.zeros((self.slots, 64))
        v[self.slot, self.lane] = flat
        for p in self.perms:
            v = v + v[:, p]
        total = v[0, 0]
        for s in range(1, self.slots):
            total = total + v[s, 0]
        return float(total)


def posteriors_one(models, seq, ln_switch):
    """one stream under the class loop of models = [(pi, A, B)] -> dict post (T, K), log_prob, status"""
    models = [tuple(np.asarray(x, dtype=np.float64) for x in m) for m in models]
    seq = np.asarray(seq, dtype=np.int64)
    K, T, M = len(models), len(seq), models[0][2].shape[1]
    Ns = [len(m[0]) for m in models]
    if T == 0:
        return _result(0, K, 0)
    GS = _Sum(Ns)
    assert GS.slots <= MAX_SLOTS
    sw = math.exp(float(ln_switch))
    runs = []  # consecutive classes of one N, computed at once: pi (Kb, N), A (Kb, N, N), B (Kb, N, M)
    for k, m in enumerate(models):
        if runs and runs[-1][0] == Ns[k]:
            runs[-1][1].append(m)
        else:
            runs.append((Ns[k], [m]))
    runs = [tuple(np.stack([m[i] for m in ms]) for i in range(3)) for _N, ms in runs]
    ent = [sw * pi for pi, _A, _B in runs]
    flat = lambda xs: np.concatenate([x.ravel() for x in xs])
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
            x = []
            for (pi, A, B), a, e in zip(runs, ah, ent):
                prod = a[:, :, None] * A  # prod[k, i, j] = ah[k][i] * A_k[i][j]
                acc = prod[:, 0, :].copy()
                for i in range(1, A.shape[1]):
                    np.add(acc, prod[:, i, :], out=acc)
                x.append((acc + e) * B[:, :, o])
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
        rows = []
        for a, b in zip(ahs[t], bh):
            g = a * b
            s = g[:, 0].copy()
            for j in range(1, g.shape[1]):
                np.add(s, g[:, j], out=s)
            rows.append(s)
        post[t] = np.concatenate(rows)
        if t == 0:
            break
        o = seq[t]
        u = [(B[:, :, o] * b) / cs[t] for (_pi, _A, B), b in zip(runs, bh)]
        r = sw * GS(flat([pi * v for (pi, _A, _B), v in zip(runs, u)]))
        bh = []
        for (_pi, A, _B), v in zip(runs, u):
            prod = A * v[:, None, :]  # prod[k, i, j] = A_k[i][j] * u[k][j]
            acc = prod[:, :, 0].copy()
            for j in range(1, A.shape[1]):
                np.add(acc, prod[:, :, j], out=acc)
            bh.append(acc + r)
    return dict(post=post, log_prob=log_prob(p, E), status=0)


def posteriors(models, sym, offs, ln_switch):
    """the layout of ecoz2rs_amd.hmm.segment_posteriors: post (sum T_s, K), per stream log_prob and status"""
    sym = np.asarray(sym)
    K = len(models)
    outs = [posteriors_one(models, sym[a:b], ln_switch) for a, b in zip(offs[:-1], offs[1:])]
    return dict(post=np.concatenate([o["post"] for o in outs]) if outs else np.zeros((0, K)),
                log_prob=np.array([o["log_prob"] for o in outs], dtype=np.float64),
                status=np.array([o["status"] for o in outs], dtype=np.int32))


def transcribe(models, seq, ln_switch):
    """the contract of DESIGN.md 4.8.7, literally: -> (post as T lists of K floats, ln P(O | loop), status)"""
    K = len(models)
    Ns = [len(m[0]) for m in models]
    M = len(models[0][2][0])
    pi = [[float(m[0][j]) for j in range(N)] for m, N in zip(models, Ns)]
    A = [[[float(m[1][i][j]) for j in range(N)] for i in range(N)] for m, N in zip(models, Ns)]
    B = [[[float(m[2][j][o]) for o in range(M)] for j in range(N)] for m, N in zip(models, Ns)]
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

    sw = math.exp(float(ln_switch))
    e = [[sw * pi[k][j] for j in range(Ns[k])] for k in range(K)]
    ahs, cs = [], []
    p, E = 0.5, 1
    for t in range(T):
        if o[t] >= M:
            return zero, NINF, 2
        if t == 0:
            x = [[pi[k][j] * B[k][j][o[0]] for j in range(Ns[k])] for k in range(K)]
        else:
            ah = ahs[-1]
            x = []
            for k in range(K):
                xk = []
                for j in range(Ns[k]):
                    acc = ah[k][0] * A[k][0][j]
                    for i in range(1, Ns[k]):
                        acc = acc + ah[k][i] * A[k][i][j]
                    xk.append((acc + e[k][j]) * B[k][j][o[t]])
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
        row = []
        for k in range(K):
            s = ahs[t][k][0] * bh[k][0]
            for j in range(1, Ns[k]):
                s = s + ahs[t][k][j] * bh[k][j]
            row.append(s)
        post[t] = row
        if t == 0:
            break
        u = [[(B[k][j][o[t]] * bh[k][j]) / cs[t] for j in range(Ns[k])] for k in range(K)]
        r = sw * GS([[pi[k][j] * u[k][j] for j in range(Ns[k])] for k in range(K)])
        nb = []
        for k in range(K):
            bk = []
            for i in range(Ns[k]):
                acc = A[k][i][0] * u[k][0]
                for j in range(1, Ns[k]):
                    acc = acc + A[k][i][j] * u[k][j]
                bk.append(acc + r)
            nb.append(bk)
        bh = nb
    return post, log_prob(p, E), 0


def segment_posteriors(cls, entered, post):
    """[(mean, min)] of post[t][class of the segment] over the frames of each segment of one stream: a serial sum in frame
    order, then one division (the host arithmetic of the report)"""
    T = len(cls)
    starts = [t for t in range(T) if entered[t]]
    out = []
    for b, e in zip(starts, starts[1:] + [T]):
        k = int(cls[b])
        s, lo = 0.0, float(post[b][k])
        for t in range(b, e):
            v = float(post[t][k])
            s = s + v
            lo = v if v < lo else lo
        out.append((s / float(e - b), lo))
    return out
