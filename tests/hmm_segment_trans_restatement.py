"""numpy restatement of the joint Viterbi under class-to-class prices (TEST INFRASTRUCTURE): e2vq_hmm_segment_trans and
`hmm segment --class-transitions`, DESIGN.md 4.8.8.

The logarithms are hmm_viterbi_restatement's.  Every step is one IEEE double addition or comparison; np.argmax returns the
first maximum, which is the contract's strict `>` with the lowest index winning ties -- over a class's d the lowest state,
over the sources of a destination the lowest class.  `transcribe` is the contract written out literally in plain loops.
"""
import numpy as np

from .hmm_viterbi_restatement import NINF, log_model

ENTER = -1


def _empty_result(T, status):
    if status == 2:
        g = np.full(T, NINF)
        g[0] = 0.0
        return dict(cls=np.full(T, 0xFFFF, np.uint16), state=np.full(T, 0xFFFF, np.uint16), entered=np.zeros(T, np.uint8),
                    exit_score=g, log_prob=NINF, status=2)
    return dict(cls=np.zeros(0, np.uint16), state=np.zeros(0, np.uint16), entered=np.zeros(0, np.uint8),
                exit_score=np.zeros(0), log_prob=0.0, status=0)


def segment_trans_logs(lms, seq, lt):
    """one stream under the class loop of the models' logarithms lms = [(lpi, lA, lB)] and the K x K prices lt -> dict
    cls, state, entered, exit_score, log_prob, status"""
    seq = np.asarray(seq, dtype=np.int64)
    lt = np.asarray(lt, dtype=np.float64)
    K = len(lms)
    M = lms[0][2].shape[1]
    T = len(seq)
    if T == 0:
        return _empty_result(0, 0)
    if np.any(seq >= M):
        return _empty_result(T, 2)
    Ns = [len(m[0]) for m in lms]
    comp0 = np.concatenate([[0], np.cumsum(Ns)])
    owner = np.concatenate([np.full(N, k) for k, N in enumerate(Ns)])
    lpi = np.concatenate([m[0] for m in lms])
    d = np.concatenate([m[0] + m[2][:, seq[0]] for m in lms])
    psi = np.zeros((T, len(d)), dtype=np.int64)
    src = np.zeros((T, K), dtype=np.int64)
    xs = np.zeros((T, K), dtype=np.int64)
    Es = np.zeros((T, K))
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            parts = [d[comp0[k]:comp0[k + 1]] for k in range(K)]
            x = np.array([int(np.argmax(p)) for p in parts])
            E = np.array([p[i] for p, i in zip(parts, x)])
            v = E[:, None] + lt  # v[f, k] = E[f] + lt[f][k]
            s = np.argmax(v, axis=0)
            base = v[s, np.arange(K)]
            xs[t], Es[t], src[t] = x, E, s
            enter = base[owner] + lpi
            nd = np.empty_like(d)
            for k, (_lpi, lA, lB) in enumerate(lms):
                a, b = comp0[k], comp0[k + 1]
                w = parts[k][:, None] + lA  # w[i, j] = d[k][i] + lA_k[i][j]
                arg = np.argmax(w, axis=0)
                best = w[arg, np.arange(b - a)]
                ent = enter[a:b] > best
                psi[t, a:b] = np.where(ent, ENTER, arg)
                nd[a:b] = np.where(ent, enter[a:b], best) + lB[:, seq[t]]
            d = nd
    q = int(np.argmax(d))
    lp = float(d[q])
    cls, state, entered = np.zeros(T, np.uint16), np.zeros(T, np.uint16), np.zeros(T, np.uint8)
    ex = np.zeros(T)
    for t in range(T - 1, -1, -1):
        k = int(owner[q])
        cls[t], state[t] = k, q - comp0[k]
        if t == 0:
            entered[0] = 1
            break
        a = psi[t, q]
        f = k
        if a == ENTER:
            entered[t] = 1
            f = int(src[t, k])
            q = int(comp0[f] + xs[t, f])
        else:
            q = int(comp0[k] + a)
        ex[t] = Es[t, f]
    return dict(cls=cls, state=state, entered=entered, exit_score=ex, log_prob=lp, status=1 if lp == NINF else 0)


def segment_trans(models, sym, offs, lt):
    """the layout of ecoz2rs_amd.hmm.segment_trans without `segments`: per-frame arrays concatenated, per-stream arrays"""
    lms = [log_model(*m) for m in models]
    sym = np.asarray(sym)
    outs = [segment_trans_logs(lms, sym[a:b], lt) for a, b in zip(offs[:-1], offs[1:])]
    cat = lambda key, dt: np.concatenate([o[key] for o in outs]).astype(dt) if outs else np.zeros(0, dt)
    return dict(cls=cat("cls", np.uint16), state=cat("state", np.uint16), entered=cat("entered", np.uint8),
                exit_score=cat("exit_score", np.float64), log_prob=np.array([o["log_prob"] for o in outs], dtype=np.float64),
                status=np.array([o["status"] for o in outs], dtype=np.int32))


def transcribe(models, seq, lt, want_d=False):
    """the contract of DESIGN.md 4.8.8, literally: -> (cls list, state list, entered list, exit_score list, ln P*, status),
    and with want_d the list over t of d_t as [[d_t[k][j]]]"""
    import math
    lg = lambda x: math.log(x) if x > 0.0 else NINF
    K = len(models)
    Ns = [len(m[0]) for m in models]
    M = len(models[0][2][0])
    lpi = [[lg(float(m[0][j])) for j in range(N)] for m, N in zip(models, Ns)]
    lA = [[[lg(float(m[1][i][j])) for j in range(N)] for i in range(N)] for m, N in zip(models, Ns)]
    lB = [[[lg(float(m[2][j][o])) for o in range(M)] for j in range(N)] for m, N in zip(models, Ns)]
    lt = [[float(lt[f][k]) for k in range(K)] for f in range(K)]
    o = [int(x) for x in seq]
    T = len(o)
    if T == 0:
        return ([], [], [], [], 0.0, 0) + (([],) if want_d else ())
    if any(x >= M for x in o):
        return ([0xFFFF] * T, [0xFFFF] * T, [0] * T, [0.0] + [NINF] * (T - 1), NINF, 2) + (([],) if want_d else ())
    d = [[lpi[k][j] + lB[k][j][o[0]] for j in range(Ns[k])] for k in range(K)]
    ds = [d]
    psi, srcs, xss, Ess = [None], [None], [None], [None]
    for t in range(1, T):
        E, x = [0.0] * K, [0] * K
        for f in range(K):
            E[f], x[f] = d[f][0], 0
            for i in range(1, Ns[f]):
                if d[f][i] > E[f]:
                    E[f], x[f] = d[f][i], i
        base, src = [0.0] * K, [0] * K
        for k in range(K):
            base[k], src[k] = E[0] + lt[0][k], 0
            for f in range(1, K):
                v = E[f] + lt[f][k]
                if v > base[k]:
                    base[k], src[k] = v, f
        nd, rows = [], []
        for k in range(K):
            ndk, row = [0.0] * Ns[k], [0] * Ns[k]
            for j in range(Ns[k]):
                best, arg = d[k][0] + lA[k][0][j], 0
                for i in range(1, Ns[k]):
                    v = d[k][i] + lA[k][i][j]
                    if v > best:
                        best, arg = v, i
                xe = base[k] + lpi[k][j]
                if xe > best:
                    best, arg = xe, ENTER
                ndk[j] = best + lB[k][j][o[t]]
                row[j] = arg
            nd.append(ndk)
            rows.append(row)
        d = nd
        ds.append(d)
        psi.append(rows)
        srcs.append(src)
        xss.append(x)
        Ess.append(E)
    best, q = None, None
    for k in range(K):
        for j in range(Ns[k]):
            if best is None or d[k][j] > best:
                best, q = d[k][j], (k, j)
    cls, state, entered, ex = [0] * T, [0] * T, [0] * T, [0.0] * T
    for t in range(T - 1, -1, -1):
        cls[t], state[t] = q
        if t == 0:
            entered[0] = 1
            break
        a = psi[t][q[0]][q[1]]
        if a == ENTER:
            entered[t] = 1
            f = srcs[t][q[0]]
            q = (f, xss[t][f])
        else:
            q = (q[0], a)
        ex[t] = Ess[t][q[0]]
    out = (cls, state, entered, ex, best, (1 if best == NINF else 0))
    return out + ((ds,) if want_d else ())


def segments_of(cls, entered, exit_score, log_prob, lt):
    """[(begin, end, class, log_prob)] of one stream: the host arithmetic of the contract"""
    lt = np.asarray(lt, dtype=np.float64)
    T = len(cls)
    starts = [t for t in range(T) if entered[t]]
    out = []
    for b, e in zip(starts, starts[1:] + [T]):
        hi = np.float64(log_prob if e == T else exit_score[e])
        with np.errstate(invalid="ignore"):
            lo = np.float64(0.0) if b == 0 else np.float64(exit_score[b]) + lt[int(cls[b - 1]), int(cls[b])]
            out.append((b, e, int(cls[b]), float(hi - lo)))
    return out
