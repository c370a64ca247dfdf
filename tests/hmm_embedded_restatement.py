"""numpy restatement of embedded (transcript-constrained) Baum-Welch (TEST INFRASTRUCTURE): e2vq_hmm_embedded_estep,
e2vq_hmm_train_embedded and `hmm learn --embedded`, DESIGN.md 4.8.11.

The arithmetic is linear and scaled; every operation is one IEEE double operation in the contract's order (numpy forms no
fma).  sw = math.exp(ln_switch) is the C library's exp, as on the host.  `transcribe` is the contract written out literally
in plain Python loops; `estep_one` is the same operations vectorised over the units of one N and sequential in t and along
every chain.  The global sum depends on the packing of the stream's units into wave-slots of 64 lanes
(hmm_posterior_restatement.packing): per slot a butterfly over the 64 lanes with idle lanes at 0.0, then the slots in order.
The counts are the int64 limb pairs of fix2 (restated here), one block per class in the layout of e2vq_hmm_acc_words.
"""
import math

import numpy as np

from .hmm_posterior_restatement import log_prob, packing, scale_step

NINF = float("-inf")
MAX_SLOTS = 16
ACC_SHIFT = 29
MAX_ESTEPS = 1000


def acc_words(N, M):
    return 2 * (N + N * N + N + N * M + N) + 2


def layout(N, M):
    """word offsets of PI, AN, AD, BN, BD and the two trailing counts within a class's block"""
    PI = 0
    AN = PI + 2 * N
    AD = AN + 2 * N * N
    BN = AD + 2 * N
    BD = BN + 2 * N * M
    return dict(PI=PI, AN=AN, AD=AD, BN=BN, BD=BD, used=BD + 2 * N, skipped=BD + 2 * N + 1)


def fix2(x):
    """e2vq::fix2(x, ACC_SHIFT): -> (hi, lo) as int64 (arrays)"""
    y = np.ldexp(np.asarray(x, dtype=np.float64), ACC_SHIFT)
    h = np.rint(y)
    lo = np.rint(np.ldexp(y - h, 31))
    return h.astype(np.int64), lo.astype(np.int64)


def unfix(hi, lo):
    """e2vq::unfix(hi, lo, ACC_SHIFT): the exact integer rounded once to the nearest double (Python's int / int is)"""
    return (int(hi) * (1 << 31) + int(lo)) / (1 << (ACC_SHIFT + 31))


def decode(acc, N, M):
    """a class's words -> dict of float arrays PI, AN, AD, BN, BD and the ints used, skipped"""
    lay = layout(N, M)
    cell = lambda at, n: np.array([unfix(acc[at + 2 * i], acc[at + 2 * i + 1]) for i in range(n)])
    return dict(PI=cell(lay["PI"], N), AN=cell(lay["AN"], N * N).reshape(N, N), AD=cell(lay["AD"], N),
                BN=cell(lay["BN"], N * M).reshape(N, M), BD=cell(lay["BD"], N), used=int(acc[lay["used"]]),
                skipped=int(acc[lay["skipped"]]))


def _sets(L, optional):
    opt = [bool(optional[l]) if optional is not None else False for l in range(L)]
    S0 = [0] + ([1] if opt[0] and L > 1 else [])
    F = [L - 1] + ([L - 2] if opt[L - 1] and L > 1 else [])
    skip = [l >= 2 and opt[l - 1] for l in range(L)]          # l - 2 is in pred(l)
    succ2 = [l + 2 < L and opt[l + 1] for l in range(L)]      # l + 2 is in succ(l)
    return S0, F, skip, succ2


def slots_of(models, units):
    return packing([len(models[k][0]) for k in units])[2]


class _GS:
    def __init__(self, uN):
        self.slot, self.lane, self.slots = packing(uN)
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


def _finish(accs, models, units, status):
    """the trailing words: the stream's mark at every class its transcript names"""
    M = models[0][2].shape[1]
    for k in sorted(set(int(u) for u in units)):
        lay = layout(len(models[k][0]), M)
        accs[k][lay["used" if status == 0 else "skipped"]] += 1


def _rowsums(accs, models):
    M = models[0][2].shape[1]
    for k, acc in enumerate(accs):
        N = len(models[k][0])
        lay = layout(N, M)
        an = acc[lay["AN"]:lay["AN"] + 2 * N * N].reshape(N, N, 2)
        acc[lay["AD"]:lay["AD"] + 2 * N] = an.sum(axis=1).ravel()


def estep_one(models, seq, units, optional, ln_switch, accs):
    """one stream; adds its counts to accs (a list of int64 word arrays, one per class; AD is left to _rowsums)
    -> (log_prob, status)"""
    models = [tuple(np.asarray(x, dtype=np.float64) for x in m) for m in models]
    seq = np.asarray(seq, dtype=np.int64)
    units = [int(u) for u in units]
    T, L, M = len(seq), len(units), models[0][2].shape[1]
    uN = [len(models[k][0]) for k in units]
    GS = _GS(uN)
    assert GS.slots <= MAX_SLOTS

    def fail(status):
        _finish(accs, models, units, status)
        return NINF, status

    if T < 1:
        return fail(1)
    S0, F, skip, succ2 = _sets(L, optional)
    skip_idx = np.flatnonzero(skip)
    succ2_idx = np.flatnonzero(succ2)
    sw = math.exp(float(ln_switch))
    comp0 = np.concatenate([[0], np.cumsum(uN)])[:-1]
    sumN = int(sum(uN))
    groups = []  # the units of one N, computed at once
    for N in sorted(set(uN)):
        idx = np.array([l for l in range(L) if uN[l] == N])
        cls = np.array([units[l] for l in idx])
        pi = np.stack([models[k][0] for k in cls])
        A = np.stack([models[k][1] for k in cls])
        B = np.stack([models[k][2] for k in cls])
        lay = layout(N, M)
        groups.append(dict(N=N, idx=idx, cls=cls, pi=pi, e=sw * pi, A=A, B=B, lay=lay,
                           pos=(comp0[idx][:, None] + np.arange(N)[None, :]),
                           init=np.isin(idx, S0)[:, None], fin=np.isin(idx, F)[:, None]))

    def flat(xs):
        out = np.zeros(sumN)
        for g, x in zip(groups, xs):
            out[g["pos"]] = x
        return out

    def chain_last(x):  # sum over the last axis in index order
        s = x[..., 0].copy()
        for j in range(1, x.shape[-1]):
            s = s + x[..., j]
        return s

    ahs, ms, cs = [], [], []
    p, E = 0.5, 1
    ah = None
    for t in range(T):
        o = seq[t]
        if o >= M:
            return fail(2)
        if t == 0:
            x = [np.where(g["init"], g["pi"] * g["B"][:, :, o], 0.0) for g in groups]
            m = [np.zeros_like(g["pi"]) for g in groups]
        else:
            V = np.zeros(L)  # the normalised mass of every unit at t - 1, in state order
            for g, a in zip(groups, ah):
                V[g["idx"]] = chain_last(a)
            q = np.zeros(L)
            q[1:] = V[:-1]
            q[skip_idx] = q[skip_idx] + V[skip_idx - 2]
            x, m = [], []
            for g, a in zip(groups, ah):
                prod = a[:, :, None] * g["A"]
                acc = prod[:, 0, :].copy()
                for i in range(1, g["N"]):
                    acc = acc + prod[:, i, :]
                mg = q[g["idx"]][:, None] * g["e"]
                m.append(mg)
                x.append((acc + mg) * g["B"][:, :, o])
        c = GS(flat(x))
        if not c > 0.0:
            return fail(1)
        ah = [xg / c for xg in x]
        ahs.append(ah)
        ms.append(m)
        cs.append(c)
        p, E = scale_step(c, p, E)
    Z = GS(flat([np.where(g["fin"], a, 0.0) for g, a in zip(groups, ah)]))
    if not Z > 0.0:
        return fail(1)
    p, E = scale_step(Z, p, E)

    def add(k_arr, at, val):  # val (U, ...) -> the cells `at` (U, ...) of the units' classes
        hi, lo = fix2(val)
        for r, k in enumerate(k_arr):
            np.add.at(accs[k], at[r].ravel(), hi[r].ravel())
            np.add.at(accs[k], at[r].ravel() + 1, lo[r].ravel())

    zinv = 1.0 / Z
    bh = [np.where(g["fin"], zinv, 0.0) * np.ones_like(g["pi"]) for g in groups]
    for t in range(T - 1, -1, -1):
        o = seq[t]
        for g, a, b in zip(groups, ahs[t], bh):
            N, lay = g["N"], g["lay"]
            U = len(g["idx"])
            gam = a * b
            j = np.arange(N)[None, :].repeat(U, 0)
            add(g["cls"], lay["BN"] + 2 * (j * M + o), gam)
            add(g["cls"], lay["BD"] + 2 * j, gam)
            if t == 0:
                add(g["cls"], lay["PI"] + 2 * j, gam)
        if t == 0:
            break
        u = [(g["B"][:, :, o] * b) / cs[t] for g, b in zip(groups, bh)]
        R = np.zeros(L)
        for g, ug in zip(groups, u):
            R[g["idx"]] = chain_last(g["e"] * ug)
        r = np.zeros(L)
        r[:-1] = R[1:]
        r[succ2_idx] = r[succ2_idx] + R[succ2_idx + 2]
        nb = []
        for g, ug, mg, ap in zip(groups, u, ms[t], ahs[t - 1]):
            N, lay = g["N"], g["lay"]
            U = len(g["idx"])
            j = np.arange(N)[None, :].repeat(U, 0)
            has_pred = (g["idx"] >= 1)[:, None]
            add(g["cls"], lay["PI"] + 2 * j, np.where(has_pred, mg * ug, 0.0))
            xi = (ap[:, :, None] * g["A"]) * ug[:, None, :]
            ij = (np.arange(N)[:, None] * N + np.arange(N)[None, :])[None].repeat(U, 0)
            add(g["cls"], lay["AN"] + 2 * ij, xi)
            prod = g["A"] * ug[:, None, :]
            acc = prod[:, :, 0].copy()
            for jj in range(1, N):
                acc = acc + prod[:, :, jj]
            last = (g["idx"] == L - 1)[:, None]
            nb.append(np.where(last, acc, acc + r[g["idx"]][:, None]))
        bh = nb
    _finish(accs, models, units, 0)
    return log_prob(p, E), 0


def _streams(sym, offs, units, unit_offs, optional):
    sym = np.asarray(sym)
    for s in range(len(offs) - 1):
        a, b, ua, ub = offs[s], offs[s + 1], unit_offs[s], unit_offs[s + 1]
        yield sym[a:b], np.asarray(units[ua:ub]), (None if optional is None else np.asarray(optional[ua:ub]))


def estep(models, sym, offs, units, unit_offs, optional=None, ln_switch=0.0, one=estep_one):
    """the layout of ecoz2rs_amd.hmm.embedded_estep: acc (per class its words), per stream log_prob and status"""
    M = np.asarray(models[0][2]).shape[1]
    accs = [np.zeros(acc_words(len(m[0]), M), dtype=np.int64) for m in models]
    lps, sts = [], []
    for seq, u, opt in _streams(sym, offs, units, unit_offs, optional):
        lp, st = one(models, seq, u, opt, ln_switch, accs)
        lps.append(lp)
        sts.append(st)
    _rowsums(accs, models)
    return dict(acc=accs, log_prob=np.array(lps, dtype=np.float64), status=np.array(sts, dtype=np.int32))


def adjustb_row(row, epsilon):
    row = np.where(row < epsilon, epsilon, row)
    s = 0.0
    for v in row:
        s = s + float(v)
    return row / s


def mstep(models, accs, epsilon):
    """the M-step of the contract -> new models"""
    out = []
    for (pi, A, B), acc in zip(models, accs):
        pi, A, B = (np.array(x, dtype=np.float64) for x in (pi, A, B))
        N, M = B.shape
        lay = layout(N, M)
        cell = lambda name, i: (acc[lay[name] + 2 * i], acc[lay[name] + 2 * i + 1])
        den = unfix(sum(int(cell("PI", j)[0]) for j in range(N)), sum(int(cell("PI", j)[1]) for j in range(N)))
        if den > 0.0:
            for j in range(N):
                pi[j] = unfix(*cell("PI", j)) / den
        for i in range(N):
            den = unfix(*cell("AD", i))
            if den > 0.0:
                for j in range(N):
                    A[i, j] = unfix(*cell("AN", i * N + j)) / den
        for j in range(N):
            den = unfix(*cell("BD", j))
            if den > 0.0:
                for k in range(M):
                    B[j, k] = unfix(*cell("BN", j * M + k)) / den
        if epsilon > 0.0 and acc[lay["used"]] > 0:
            for j in range(N):
                B[j] = adjustb_row(B[j], epsilon)
        out.append((pi, A, B))
    return out


def train(models, sym, offs, units, unit_offs, optional=None, ln_switch=0.0, epsilon=1e-5, val_auto=0.3, max_iterations=-1):
    """the loop of the contract -> (models, [sum ln P per E-step]); raises ValueError where the call returns 1"""
    models = [tuple(np.array(x, dtype=np.float64) for x in m) for m in models]
    hist, Lprev, it = [], 0.0, 0
    while True:
        if (max_iterations >= 0 and it >= max_iterations) or it >= MAX_ESTEPS:
            break
        r = estep(models, sym, offs, units, unit_offs, optional, ln_switch)
        L = 0.0
        for lp, st in zip(r["log_prob"], r["status"]):
            if st == 0:
                L = L + float(lp)
        if it == 0 and not (r["status"] == 0).any():
            raise ValueError("no stream can be explained by its transcript")
        hist.append(L)
        if it > 0 and L - Lprev <= val_auto:
            break
        models = mstep(models, r["acc"], epsilon)
        Lprev = L
        it += 1
    return models, hist


def transcribe(models, seq, units, optional, ln_switch, accs):
    """the contract of DESIGN.md 4.8.11, literally, for one stream: adds to accs as estep_one does -> (log_prob, status)"""
    units = [int(u) for u in units]
    L, T = len(units), len(seq)
    M = len(models[0][2][0])
    Nk = [len(m[0]) for m in models]
    pi = [[float(models[k][0][j]) for j in range(Nk[k])] for k in units]
    A = [[[float(models[k][1][i][j]) for j in range(Nk[k])] for i in range(Nk[k])] for k in units]
    B = [[[float(models[k][2][j][o]) for o in range(M)] for j in range(Nk[k])] for k in units]
    uN = [Nk[k] for k in units]
    o = [int(x) for x in seq]
    slot, lane, slots = packing(uN)
    comp0 = [sum(uN[:l]) for l in range(L)]

    def GS(x):
        v = [[0.0] * 64 for _ in range(slots)]
        for l in range(L):
            for j in range(uN[l]):
                v[slot[comp0[l] + j]][lane[comp0[l] + j]] = x[l][j]
        for mk in (32, 16, 8, 4, 2, 1):
            v = [[row[q] + row[q ^ mk] for q in range(64)] for row in v]
        total = v[0][0]
        for s in range(1, slots):
            total = total + v[s][0]
        return total

    def fail(status):
        _finish(accs, models, units, status)
        return NINF, status

    if T < 1:
        return fail(1)
    S0, F, skip, succ2 = _sets(L, optional)
    sw = math.exp(float(ln_switch))
    e = [[sw * pi[l][j] for j in range(uN[l])] for l in range(L)]
    ahs, ms, cs = [], [], []
    p, E = 0.5, 1
    for t in range(T):
        if o[t] >= M:
            return fail(2)
        x, m = [], []
        V = []  # the normalised mass of every unit at t - 1
        for l in range(L if t > 0 else 0):
            s = ahs[-1][l][0]
            for j in range(1, uN[l]):
                s = s + ahs[-1][l][j]
            V.append(s)
        for l in range(L):
            xl, ml = [], []
            for j in range(uN[l]):
                if t == 0:
                    xl.append(pi[l][j] * B[l][j][o[0]] if l in S0 else 0.0)
                    ml.append(0.0)
                    continue
                acc = ahs[-1][l][0] * A[l][0][j]
                for i in range(1, uN[l]):
                    acc = acc + ahs[-1][l][i] * A[l][i][j]
                if l >= 1:
                    inn = V[l - 1]
                    if skip[l]:
                        inn = inn + V[l - 2]
                    mm = inn * e[l][j]
                    ml.append(mm)
                    xl.append((acc + mm) * B[l][j][o[t]])
                else:
                    ml.append(0.0)
                    xl.append(acc * B[l][j][o[t]])
            x.append(xl)
            m.append(ml)
        c = GS(x)
        if not c > 0.0:
            return fail(1)
        ahs.append([[v / c for v in xl] for xl in x])
        ms.append(m)
        cs.append(c)
        p, E = scale_step(c, p, E)
    Z = GS([[ahs[-1][l][j] if l in F else 0.0 for j in range(uN[l])] for l in range(L)])
    if not Z > 0.0:
        return fail(1)
    p, E = scale_step(Z, p, E)

    def put(l, at, val):
        hi, lo = fix2(val)
        accs[units[l]][at] += int(hi)
        accs[units[l]][at + 1] += int(lo)

    lays = [layout(uN[l], M) for l in range(L)]
    bh = [[1.0 / Z if l in F else 0.0 for _ in range(uN[l])] for l in range(L)]
    for t in range(T - 1, -1, -1):
        for l in range(L):
            for j in range(uN[l]):
                g = ahs[t][l][j] * bh[l][j]
                put(l, lays[l]["BN"] + 2 * (j * M + o[t]), g)
                put(l, lays[l]["BD"] + 2 * j, g)
                if t == 0:
                    put(l, lays[l]["PI"] + 2 * j, g)
        if t == 0:
            break
        u = [[(B[l][j][o[t]] * bh[l][j]) / cs[t] for j in range(uN[l])] for l in range(L)]
        R = []
        for l in range(L):
            s = e[l][0] * u[l][0]
            for j in range(1, uN[l]):
                s = s + e[l][j] * u[l][j]
            R.append(s)
        nb = []
        for l in range(L):
            N = uN[l]
            for j in range(N):
                for i in range(N):
                    put(l, lays[l]["AN"] + 2 * (i * N + j), (ahs[t - 1][l][i] * A[l][i][j]) * u[l][j])
                if l >= 1:
                    put(l, lays[l]["PI"] + 2 * j, ms[t][l][j] * u[l][j])
            bl = []
            for i in range(N):
                acc = A[l][i][0] * u[l][0]
                for j in range(1, N):
                    acc = acc + A[l][i][j] * u[l][j]
                if l + 1 < L:
                    r = R[l + 1]
                    if succ2[l]:
                        r = r + R[l + 2]
                    acc = acc + r
                bl.append(acc)
            nb.append(bl)
        bh = nb
    _finish(accs, models, units, 0)
    return log_prob(p, E), 0
