"""numpy restatement of `hmm align --posteriors` (TEST INFRASTRUCTURE): e2vq_hmm_align_posteriors and
e2vq_hmm_align_unit_moments, DESIGN.md 4.8.12.

The arithmetic is linear and scaled; every operation is one IEEE double operation in the contract's order (numpy forms no
fma).  sw = math.exp(ln_switch) is the C library's exp, as on the host.  The loops over the frames, along every chain and
over the slots are plain Python loops; the units of one N are computed side by side (elementwise, so no order is lost).
GS depends on the packing of the stream's units into wave-slots of 64 lanes: per slot a butterfly over the 64 lanes with idle
lanes at 0.0, then the slots in order.  The forward pass, the status, the end and the backward pass are written out here a
second time rather than taken from hmm_embedded_restatement.py; test_hmm_align_posteriors_cpu.py holds the two against one
another on the bits of log_prob and status.
"""
import math

import numpy as np

from .hmm_posterior_restatement import log_prob, packing, scale_step

NINF = float("-inf")
MAX_SLOTS = 16
NO_UNIT = 0xFFFF


def _sets(L, optional):
    """S0, F and, per unit, whether l - 2 is in pred(l) and whether l + 2 is in succ(l)"""
    opt = [bool(optional[l]) if optional is not None else False for l in range(L)]
    S0 = [0] + ([1] if opt[0] and L > 1 else [])
    F = [L - 1] + ([L - 2] if opt[L - 1] and L > 1 else [])
    skip = [l >= 2 and opt[l - 1] for l in range(L)]
    succ2 = [l + 2 < L and opt[l + 1] for l in range(L)]
    return S0, F, skip, succ2


class _GS:
    def __init__(self, uN):
        self.slot, self.lane, self.slots = packing(uN)

    def __call__(self, flat):
        v = np.zeros((self.slots, 64))
        v[self.slot, self.lane] = flat
        for m in (32, 16, 8, 4, 2, 1):
            v = v + v[:, np.arange(64) ^ m]
        total = v[0, 0]
        for s in range(1, self.slots):
            total = total + v[s, 0]
        return float(total)


def slots_of(models, units):
    return packing([len(models[k][0]) for k in units])[2]


def _chain(x):
    """the sum over the last axis in index order"""
    s = x[..., 0].copy()
    for j in range(1, x.shape[-1]):
        s = s + x[..., j]
    return s


def posteriors_one(models, seq, units, optional=None, ln_switch=0.0, path_unit=None, ref=None):
    """one stream -> dict occ (T, L), post_path (T), w0, w1, w2 (L), log_prob, status"""
    models = [tuple(np.asarray(x, dtype=np.float64) for x in m) for m in models]
    seq = np.asarray(seq, dtype=np.int64)
    units = [int(u) for u in units]
    T, L, M = len(seq), len(units), models[0][2].shape[1]
    uN = [len(models[k][0]) for k in units]
    GS = _GS(uN)
    assert GS.slots <= MAX_SLOTS
    occ, post = np.zeros((T, L)), np.zeros(T)
    w = np.zeros((3, L))

    def result(lp, status):
        return dict(occ=occ, post_path=post, w0=w[0], w1=w[1], w2=w[2], log_prob=lp, status=status)

    if T < 1:
        return result(NINF, 1)
    ref = np.zeros(L, dtype=np.int64) if ref is None else np.asarray(ref, dtype=np.int64)
    assert ((ref >= 0) & (ref < T)).all()
    S0, F, skip, succ2 = _sets(L, optional)
    skip_idx, succ2_idx = np.flatnonzero(skip), np.flatnonzero(succ2)
    sw = math.exp(float(ln_switch))
    comp0 = np.concatenate([[0], np.cumsum(uN)])[:-1]
    sumN = int(sum(uN))
    groups = []
    for N in sorted(set(uN)):
        idx = np.array([l for l in range(L) if uN[l] == N])
        pi = np.stack([models[units[l]][0] for l in idx])
        groups.append(dict(N=N, idx=idx, pi=pi, e=sw * pi, A=np.stack([models[units[l]][1] for l in idx]),
                           B=np.stack([models[units[l]][2] for l in idx]), pos=comp0[idx][:, None] + np.arange(N)[None, :],
                           init=np.isin(idx, S0)[:, None], fin=np.isin(idx, F)[:, None]))

    def flat(xs):
        out = np.zeros(sumN)
        for g, x in zip(groups, xs):
            out[g["pos"]] = x
        return out

    # ---- forward, status, end ------------------------------------------------------------------------------------------------
    ahs, ms, cs = [], [], []
    p, E = 0.5, 1
    ah = None
    for t in range(T):
        o = seq[t]
        if o >= M:
            return result(NINF, 2)
        if t == 0:
            x = [np.where(g["init"], g["pi"] * g["B"][:, :, o], 0.0) for g in groups]
            m = [np.zeros_like(g["pi"]) for g in groups]
        else:
            V = np.zeros(L)
            for g, a in zip(groups, ah):
                V[g["idx"]] = _chain(a)
            q = np.zeros(L)
            q[1:] = V[:-1]
            q[skip_idx] = q[skip_idx] + V[skip_idx - 2]
            x, m = [], []
            for g, a in zip(groups, ah):
                acc = a[:, 0, None] * g["A"][:, 0, :]
                for i in range(1, g["N"]):
                    acc = acc + a[:, i, None] * g["A"][:, i, :]
                mg = q[g["idx"]][:, None] * g["e"]  # (unit 0: q = 0.0, so m = 0.0 and acc + m has the bits of acc)
                m.append(mg)
                x.append((acc + mg) * g["B"][:, :, o])
        c = GS(flat(x))
        if not c > 0.0:
            return result(NINF, 1)
        ah = [xg / c for xg in x]
        ahs.append(ah)
        ms.append(m)
        cs.append(c)
        p, E = scale_step(c, p, E)
    Z = GS(flat([np.where(g["fin"], a, 0.0) for g, a in zip(groups, ah)]))
    if not Z > 0.0:
        return result(NINF, 1)
    p, E = scale_step(Z, p, E)

    # ---- backward: occupancy, entries, the descending sums ----------------------------------------------------------------------
    zinv = 1.0 / Z
    bh = [np.where(g["fin"], zinv, 0.0) * np.ones_like(g["pi"]) for g in groups]
    for t in range(T - 1, -1, -1):
        o = seq[t]
        G = np.zeros(L)
        for g, a, b in zip(groups, ahs[t], bh):
            G[g["idx"]] = _chain(a * b)
        occ[t] = G
        if path_unit is not None and int(path_unit[t]) != NO_UNIT and int(path_unit[t]) < L:
            post[t] = G[int(path_unit[t])]
        if t == 0:
            En = G
        else:
            u = [(g["B"][:, :, o] * b) / cs[t] for g, b in zip(groups, bh)]
            En = np.zeros(L)
            for g, ug, mg in zip(groups, u, ms[t]):
                En[g["idx"]] = _chain(mg * ug)
            En[0] = 0.0
        d = (t - ref).astype(np.float64)
        w[0] = w[0] + En
        w[1] = w[1] + d * En
        w[2] = w[2] + (d * d) * En
        if t == 0:
            break
        R = np.zeros(L)
        for g, ug in zip(groups, u):
            R[g["idx"]] = _chain(g["e"] * ug)
        r = np.zeros(L)
        r[:-1] = R[1:]
        r[succ2_idx] = r[succ2_idx] + R[succ2_idx + 2]
        nb = []
        for g, ug in zip(groups, u):
            acc = g["A"][:, :, 0] * ug[:, 0, None]
            for j in range(1, g["N"]):
                acc = acc + g["A"][:, :, j] * ug[:, j, None]
            last = (g["idx"] == L - 1)[:, None]
            nb.append(np.where(last, acc, acc + r[g["idx"]][:, None]))
        bh = nb
    return result(log_prob(p, E), 0)


def unit_moments(w0, w1, w2, ref=None):
    """the host arithmetic -> (present, begin_mean, begin_sd)"""
    n = len(w0)
    present, mean, sd = np.array(w0, dtype=np.float64), np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        a, b, c = np.float64(w0[i]), np.float64(w1[i]), np.float64(w2[i])
        if a > 0.0:
            q = b / a
            mean[i] = np.float64(0 if ref is None else int(ref[i])) + q
            v = c / a - q * q
            sd[i] = math.sqrt(v if v > 0.0 else 0.0)
    return present, mean, sd


def posteriors(models, sym, offs, units, unit_offs, optional=None, ln_switch=0.0, path_unit=None, ref=None):
    """the layout of ecoz2rs_amd.hmm.align_posteriors"""
    sym = np.asarray(sym)
    S = len(offs) - 1
    outs = []
    for s in range(S):
        a, b, ua, ub = int(offs[s]), int(offs[s + 1]), int(unit_offs[s]), int(unit_offs[s + 1])
        outs.append(posteriors_one(models, sym[a:b], units[ua:ub], None if optional is None else optional[ua:ub], ln_switch,
                                   None if path_unit is None else path_unit[a:b], None if ref is None else ref[ua:ub]))
    cat = lambda k, dt=np.float64: np.concatenate([np.atleast_1d(o[k]) for o in outs]).astype(dt) if outs else np.zeros(0, dt)
    w0, w1, w2 = cat("w0"), cat("w1"), cat("w2")
    present, mean, sd = unit_moments(w0, w1, w2, None if ref is None else ref[:len(w0)])
    return dict(occ=[o["occ"] for o in outs], post_path=cat("post_path"), w0=w0, w1=w1, w2=w2, present=present, begin_mean=mean,
                begin_sd=sd, log_prob=cat("log_prob"), status=cat("status", np.int32))
