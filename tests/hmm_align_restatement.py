"""numpy restatement of forced alignment to a known order of units (TEST INFRASTRUCTURE): e2vq_hmm_align and `hmm align`,
DESIGN.md 4.8.10.

The logarithms are hmm_viterbi_restatement's.  Every step is one IEEE double addition or comparison in the contract's
order; np.argmax returns the first maximum, which is the contract's strict `>` with the lowest index winning ties.  The
per-frame `score` is the host replay of the contract: the decoded path walked forwards, one addition per term.
`brute_force` enumerates every admissible path.
"""
import numpy as np

from .hmm_viterbi_restatement import NINF, log_model

ENTER_1 = -1  # entered from the unit before
ENTER_2 = -2  # entered from two units before, over an optional one


def is_initial(l, opt):
    return l == 0 or (l == 1 and bool(opt[0]))


def is_final(l, L, opt):
    return l == L - 1 or (l == L - 2 and bool(opt[L - 1]))


def _no_path(T, L, status):
    sc = np.full(T, NINF)
    if T:
        sc[0] = 0.0
    return dict(unit=np.full(T, 0xFFFF, np.uint16), state=np.full(T, 0xFFFF, np.uint16), entered=np.zeros(T, np.uint8), score=sc,
                begin=np.full(L, -1, np.int64), end=np.full(L, -1, np.int64), log_prob=NINF if status else 0.0, status=status)


def replay(lms, seq, units, opt, ln_switch, unit, state, entered):
    """the path's own cumulative score at every frame: what the host computes once the path is known"""
    T = len(seq)
    ls = np.float64(ln_switch)
    score = np.zeros(T)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            l, j = int(unit[t]), int(state[t])
            lpi, lA, lB = lms[units[l]]
            if t == 0:
                score[0] = lpi[j] + lB[j, seq[0]] if is_initial(l, opt) else NINF
            elif entered[t]:
                score[t] = ((score[t - 1] + ls) + lpi[j]) + lB[j, seq[t]]
            else:
                score[t] = (score[t - 1] + lA[int(state[t - 1]), j]) + lB[j, seq[t]]
    return score


def align_logs(lms, seq, units, opt, ln_switch):
    """one stream against its transcript under the models' logarithms lms = [(lpi, lA, lB)] -> dict unit, state, entered,
    score, begin, end, log_prob, status"""
    seq = np.asarray(seq, dtype=np.int64)
    units = [int(k) for k in units]
    L = len(units)
    opt = [0] * L if opt is None else [int(bool(x)) for x in opt]
    M = lms[0][2].shape[1]
    T = len(seq)
    if T == 0:
        return _no_path(0, L, 0)
    if np.any(seq >= M):
        return _no_path(T, L, 2)
    ls = np.float64(ln_switch)
    Ns = [len(lms[k][0]) for k in units]
    comp0 = np.concatenate([[0], np.cumsum(Ns)]).astype(np.int64)
    owner = np.concatenate([np.full(N, l) for l, N in enumerate(Ns)])
    d = np.concatenate([(lms[k][0] + lms[k][2][:, seq[0]]) if is_initial(l, opt) else np.full(Ns[l], NINF)
                        for l, k in enumerate(units)])
    psi = np.zeros((T, len(d)), dtype=np.int64)
    xs = np.zeros((T, L), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            parts = [d[comp0[l]:comp0[l + 1]] for l in range(L)]
            x = [int(np.argmax(p)) for p in parts]
            E = [p[i] for p, i in zip(parts, x)]
            xs[t] = x
            nd = np.empty_like(d)
            for l, k in enumerate(units):
                lpi, lA, lB = lms[k]
                a, b = comp0[l], comp0[l + 1]
                w = parts[l][:, None] + lA  # w[i, j] = d[l][i] + lA[i][j]
                arg = np.argmax(w, axis=0)
                best = w[arg, np.arange(b - a)]
                if l >= 1:
                    e, code = E[l - 1], ENTER_1
                    if l >= 2 and opt[l - 1] and E[l - 2] > e:
                        e, code = E[l - 2], ENTER_2
                    enter = (e + ls) + lpi
                    ent = enter > best
                    psi[t, a:b] = np.where(ent, code, arg)
                    best = np.where(ent, enter, best)
                else:
                    psi[t, a:b] = arg
                nd[a:b] = best + lB[:, seq[t]]
            d = nd
    last = np.array([is_final(int(l), L, opt) for l in owner])
    q = int(np.argmax(np.where(last, d, NINF)))
    if not last[q]:  # (every candidate is -inf: the lowest composite index among them)
        q = int(np.flatnonzero(last)[0])
    lp = float(d[q])
    unit, state, entered = np.zeros(T, np.uint16), np.zeros(T, np.uint16), np.zeros(T, np.uint8)
    begin, end = np.full(L, -1, np.int64), np.full(L, -1, np.int64)
    end[owner[q]] = T
    for t in range(T - 1, -1, -1):
        l = int(owner[q])
        unit[t], state[t] = l, q - comp0[l]
        if t == 0:
            entered[0] = 1
            begin[l] = 0
            break
        a = psi[t, q]
        if a < 0:
            f = l - 1 if a == ENTER_1 else l - 2
            entered[t] = 1
            begin[l], end[f] = t, t
            q = int(comp0[f] + xs[t, f])
        else:
            q = int(comp0[l] + a)
    score = replay(lms, seq, units, opt, ln_switch, unit, state, entered)
    assert score[T - 1:].view(np.uint64)[0] == np.array([lp]).view(np.uint64)[0], "the replay does not reach ln P*"
    return dict(unit=unit, state=state, entered=entered, score=score, begin=begin, end=end, log_prob=lp, status=1 if lp == NINF else 0)


def align(models, sym, offs, units, unit_offs, optional=None, ln_switch=0.0):
    """the layout of ecoz2rs_amd.hmm.align without `units`: per-frame and per-unit arrays concatenated, per-stream arrays"""
    lms = [log_model(*m) for m in models]
    sym = np.asarray(sym)
    outs = []
    for a, b, ua, ub in zip(offs[:-1], offs[1:], unit_offs[:-1], unit_offs[1:]):
        outs.append(align_logs(lms, sym[a:b], units[ua:ub], None if optional is None else optional[ua:ub], ln_switch))
    cat = lambda key, dt: np.concatenate([o[key] for o in outs]).astype(dt) if outs else np.zeros(0, dt)
    return dict(unit=cat("unit", np.uint16), state=cat("state", np.uint16), entered=cat("entered", np.uint8),
                score=cat("score", np.float64), begin=cat("begin", np.int64), end=cat("end", np.int64),
                log_prob=np.array([o["log_prob"] for o in outs], dtype=np.float64),
                status=np.array([o["status"] for o in outs], dtype=np.int32))


def units_of(units, begin, end, score, ln_switch):
    """[(unit, class, begin, end, score)] of one stream: the host arithmetic of the contract"""
    out = []
    ls = np.float64(ln_switch)
    for l, (k, b, e) in enumerate(zip(units, begin, end)):
        if b < 0:
            continue
        with np.errstate(invalid="ignore"):
            lo = np.float64(0.0) if b == 0 else np.float64(score[b - 1]) + ls
            out.append((l, int(k), int(b), int(e), float(np.float64(score[e - 1]) - lo)))
    return out


def brute_force(lms, seq, units, opt, ln_switch):
    """every admissible path of composite states, scored in path order with the replay's additions
    -> (the greatest score, the set of paths [(l, j)] reaching it); (-inf, all paths) when none is better"""
    seq = [int(o) for o in seq]
    units = [int(k) for k in units]
    L, T = len(units), len(seq)
    opt = [0] * L if opt is None else [int(bool(x)) for x in opt]
    ls = np.float64(ln_switch)
    best, paths = NINF, set()

    def walk(t, l, j, score, path):
        nonlocal best, paths
        if t == T - 1:
            if is_final(l, L, opt):
                if score > best:
                    best, paths = score, {tuple(path)}
                elif score == best:
                    paths.add(tuple(path))
            return
        o = seq[t + 1]
        with np.errstate(invalid="ignore"):
            lpi, lA, lB = lms[units[l]]
            for j2 in range(len(lpi)):
                walk(t + 1, l, j2, (score + lA[j, j2]) + lB[j2, o], path + [(l, j2)])
            for l2 in ([l + 1] if l + 1 < L else []) + ([l + 2] if l + 2 < L and opt[l + 1] else []):
                lpi2, _lA2, lB2 = lms[units[l2]]
                for j2 in range(len(lpi2)):
                    walk(t + 1, l2, j2, ((score + ls) + lpi2[j2]) + lB2[j2, o], path + [(l2, j2)])

    for l in range(L):
        if is_initial(l, opt):
            lpi, _lA, lB = lms[units[l]]
            for j in range(len(lpi)):
                walk(0, l, j, lpi[j] + lB[j, seq[0]], [(l, j)])
    return float(best), paths
