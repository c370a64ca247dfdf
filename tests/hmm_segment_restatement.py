"""numpy restatement of the joint Viterbi over all class HMMs (TEST INFRASTRUCTURE): e2vq_hmm_segment and `hmm segment`,
DESIGN.md 4.8.6.

The logarithms are hmm_viterbi_restatement's (math.log element by element, log 0 = -inf).  Every step of the recursion is
one IEEE double addition, vectorised per class (consecutive classes of one N at once) and sequential in t; np.argmax
returns the first maximum, which is the contract's strict `>` with the lowest index winning ties, and over the
concatenated d it is the lowest (class, state).
`transcribe` is the contract written out literally in plain Python loops.
"""
import numpy as np

from .hmm_viterbi_restatement import NINF, log_model

ENTER = -1


def _empty_result(T, status):
    if status == 2:
        g = np.full(T, NINF)
        g[0] = 0.0
        return dict(cls=np.full(T, 0xFFFF, np.uint16), state=np.full(T, 0xFFFF, np.uint16), entered=np.zeros(T, np.uint8),
                    gbest=g, log_prob=NINF, status=2)
    return dict(cls=np.zeros(0, np.uint16), state=np.zeros(0, np.uint16), entered=np.zeros(0, np.uint8), gbest=np.zeros(0),
                log_prob=0.0, status=0)


def segment_logs(lms, seq, ln_switch):
    """one stream under the class loop of the models' logarithms lms = [(lpi, lA, lB)] -> dict cls, state, entered, gbest,
    log_prob, status"""
    seq = np.asarray(seq, dtype=np.int64)
    M = lms[0][2].shape[1]
    T = len(seq)
    if T == 0:
        return _empty_result(0, 0)
    if np.any(seq >= M):
        return _empty_result(T, 2)
    Ns = [len(m[0]) for m in lms]
    comp0 = np.concatenate([[0], np.cumsum(Ns)])
    owner = np.concatenate([np.full(N, k) for k, N in enumerate(Ns)])
    ln_switch = float(ln_switch)
    # consecutive classes of one N form a block that is computed at once: lpi (Kb, N), lA (Kb, N, N), lB (Kb, N, M);
    # the blocks' d, flattened in order, is d in (class, state) order
    blocks = []
    for k, m in enumerate(lms):
        if blocks and blocks[-1][0] == Ns[k]:
            blocks[-1][1].append(m)
        else:
            blocks.append((Ns[k], [m]))
    blocks = [tuple(np.stack([m[i] for m in ms]) for i in range(3)) for _N, ms in blocks]
    d = [lpi + lB[:, :, seq[0]] for lpi, _lA, lB in blocks]
    psi = [np.zeros((T,) + lpi.shape, dtype=np.int64) for lpi, _lA, _lB in blocks]
    gsel = np.zeros(T, dtype=np.int64)
    gbest = np.zeros(T)
    for t in range(1, T):
        flat = np.concatenate([x.ravel() for x in d])
        g = int(np.argmax(flat))
        G = float(flat[g])
        gsel[t], gbest[t] = g, G
        base = G + ln_switch
        nd = []
        for bi, (lpi, lA, lB) in enumerate(blocks):
            v = d[bi][:, :, None] + lA  # v[k, i, j] = d[k][i] + lA_k[i][j]
            arg = np.argmax(v, axis=1)
            best = np.take_along_axis(v, arg[:, None, :], axis=1)[:, 0, :]
            x = base + lpi
            ent = x > best
            psi[bi][t] = np.where(ent, ENTER, arg)
            nd.append(np.where(ent, x, best) + lB[:, :, seq[t]])
        d = nd
    flat = np.concatenate([x.ravel() for x in d])
    psi = np.concatenate([p.reshape(T, -1) for p in psi], axis=1)  # (T, sumN)
    q = int(np.argmax(flat))
    lp = float(flat[q])
    cls, state, entered = np.zeros(T, np.uint16), np.zeros(T, np.uint16), np.zeros(T, np.uint8)
    for t in range(T - 1, -1, -1):
        k = int(owner[q])
        cls[t], state[t] = k, q - comp0[k]
        if t == 0:
            entered[0] = 1
            break
        a = psi[t, q]
        entered[t] = 1 if a == ENTER else 0
        q = int(gsel[t]) if a == ENTER else int(comp0[k] + a)
    return dict(cls=cls, state=state, entered=entered, gbest=gbest, log_prob=lp, status=1 if lp == NINF else 0)


def segment(models, sym, offs, ln_switch):
    """the layout of ecoz2rs_amd.hmm.segment without `segments`: per-frame arrays concatenated, per-stream arrays"""
    lms = [log_model(*m) for m in models]
    sym = np.asarray(sym)
    outs = [segment_logs(lms, sym[a:b], ln_switch) for a, b in zip(offs[:-1], offs[1:])]
    cat = lambda key, dt: np.concatenate([o[key] for o in outs]).astype(dt) if outs else np.zeros(0, dt)
    return dict(cls=cat("cls", np.uint16), state=cat("state", np.uint16), entered=cat("entered", np.uint8),
                gbest=cat("gbest", np.float64), log_prob=np.array([o["log_prob"] for o in outs], dtype=np.float64),
                status=np.array([o["status"] for o in outs], dtype=np.int32))


def transcribe(models, seq, ln_switch):
    """the contract of DESIGN.md 4.8.6, literally: -> (cls list, state list, entered list, gbest list, ln P*, status)"""
    import math
    lg = lambda x: math.log(x) if x > 0.0 else NINF
    K = len(models)
    Ns = [len(m[0]) for m in models]
    M = len(models[0][2][0])
    lpi = [[lg(float(m[0][j])) for j in range(N)] for m, N in zip(models, Ns)]
    lA = [[[lg(float(m[1][i][j])) for j in range(N)] for i in range(N)] for m, N in zip(models, Ns)]
    lB = [[[lg(float(m[2][j][o])) for o in range(M)] for j in range(N)] for m, N in zip(models, Ns)]
    o = [int(x) for x in seq]
    T = len(o)
    ln_switch = float(ln_switch)
    if T == 0:
        return [], [], [], [], 0.0, 0
    if any(x >= M for x in o):
        return [0xFFFF] * T, [0xFFFF] * T, [0] * T, [0.0] + [NINF] * (T - 1), NINF, 2
    d = [[lpi[k][j] + lB[k][j][o[0]] for j in range(Ns[k])] for k in range(K)]
    psi, gs, Gs = [None], [None], [0.0]
    for t in range(1, T):
        G, g = None, None
        for k in range(K):
            for i in range(Ns[k]):
                if G is None or d[k][i] > G:
                    G, g = d[k][i], (k, i)
        base = G + ln_switch
        nd, rows = [], []
        for k in range(K):
            ndk, row = [0.0] * Ns[k], [0] * Ns[k]
            for j in range(Ns[k]):
                best, arg = d[k][0] + lA[k][0][j], 0
                for i in range(1, Ns[k]):
                    v = d[k][i] + lA[k][i][j]
                    if v > best:
                        best, arg = v, i
                x = base + lpi[k][j]
                if x > best:
                    best, arg = x, ENTER
                ndk[j] = best + lB[k][j][o[t]]
                row[j] = arg
            nd.append(ndk)
            rows.append(row)
        d = nd
        psi.append(rows)
        gs.append(g)
        Gs.append(G)
    best, q = None, None
    for k in range(K):
        for j in range(Ns[k]):
            if best is None or d[k][j] > best:
                best, q = d[k][j], (k, j)
    cls, state, entered = [0] * T, [0] * T, [0] * T
    for t in range(T - 1, -1, -1):
        cls[t], state[t] = q
        if t == 0:
            entered[0] = 1
            break
        a = psi[t][q[0]][q[1]]
        if a == ENTER:
            entered[t] = 1
            q = gs[t]
        else:
            q = (q[0], a)
    return cls, state, entered, Gs, best, (1 if best == NINF else 0)


def segments_of(cls, entered, gbest, log_prob, ln_switch):
    """[(begin, end, class, log_prob)] of one stream: the host arithmetic of the contract"""
    T = len(cls)
    starts = [t for t in range(T) if entered[t]]
    out = []
    for b, e in zip(starts, starts[1:] + [T]):
        hi = np.float64(log_prob if e == T else gbest[e])
        lo = np.float64(0.0 if b == 0 else np.float64(gbest[b]) + np.float64(ln_switch))
        with np.errstate(invalid="ignore"):
            out.append((b, e, int(cls[b]), float(hi - lo)))
    return out
