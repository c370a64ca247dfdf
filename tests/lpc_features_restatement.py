"""numpy restatement of the LPC features of stored vectors (TEST INFRASTRUCTURE): `prd show --predictors / -k /
--cepstrum` and e2vq_lpc_features, DESIGN.md 8.1.

lpca_r (src/lpc/lpca_r_rs.rs) and lpca_get_cepstrum (src/lpc/lpca_cepstrum_rs.rs): every step an element-wise IEEE
double operation (numpy never fuses a multiply and an add), vectorised across frames, sequential in i and k.  c[0] is
math.log(math.sqrt(pe)) frame by frame (the C library's functions; numpy's own log need not be).  `show` restates the text
of prd_show_rs / Predictor::show / do_show (src/prd/mod.rs:105-225).
"""
import math

import numpy as np


def lpca_r(r):
    """-> (status (T,) int32, pe (T,), rc (T, P+1), a (T, P+1)); status 0 / 1 (r[0] == 0: nothing written, pe = 0) /
    2 (pe <= 0: rc and a as the recursion left them); rc[0] = 0."""
    r = np.asarray(r, dtype=np.float64)
    T, NC = r.shape
    status = np.where(r[:, 0] == 0.0, 1, 0).astype(np.int32)
    run = status == 0
    pe = np.where(run, r[:, 0], 0.0)
    rc = np.zeros((T, NC))
    a = np.zeros((T, NC))
    a[run, 0] = 1.0
    with np.errstate(all="ignore"):
        for k in range(1, NC):
            s = np.zeros(T)
            for i in range(1, k + 1):
                s = s - a[:, k - i] * r[:, i]
            akk = s / pe
            rc[run, k] = akk[run]
            a[run, k] = akk[run]
            for i in range(1, (k >> 1) + 1):
                ai, aj = a[:, i].copy(), a[:, k - i].copy()
                a[run, i] = (ai + akk * aj)[run]
                a[run, k - i] = (aj + akk * ai)[run]
            pe = np.where(run, pe * (1.0 - akk * akk), pe)
            failed = run & (pe <= 0.0)
            status[failed] = 2
            run = run & ~failed
    return status, pe, rc, a


def c0(pe):
    """ln(sqrt(pe)) with the C library's functions (Python's math raises where C returns -inf / NaN)."""
    if pe > 0.0:
        return math.log(math.sqrt(pe))
    if pe == 0.0:
        return -math.inf
    return math.nan


def cepstrum(a, pe, Q):
    """c (T, Q) of lpca_get_cepstrum with gain = sqrt(pe)."""
    T, NC = a.shape
    P = NC - 1
    assert Q > P
    c = np.zeros((T, Q))
    c[:, 0] = [c0(float(p)) for p in pe]
    c[:, 1] = -a[:, 1]
    with np.errstate(all="ignore"):
        for i in range(2, Q):
            s = a[:, i].copy() if i <= P else np.zeros(T)
            for k in range(1, i if i <= P else P + 1):
                s = s + (float(i - k) * c[:, i - k]) * a[:, k]
            c[:, i] = -s / float(i)
    return c


def features(r, Q=0):
    st, pe, rc, a = lpca_r(r)
    out = dict(status=st, pe=pe, rc=rc, a=a)
    if Q:
        out["c"] = cepstrum(a, pe, Q)
    return out


def rust_value(v):
    """Rust's `{:.4e}` when |v| < 0.00001, else `{:.5}`."""
    v = float(v)
    if math.isnan(v):
        return "NaN"
    if math.isinf(v):
        return "inf" if v > 0 else "-inf"
    if abs(v) < 0.00001:
        m, ex = f"{v:.4e}".split("e")
        return f"{m}e{int(ex)}"
    return f"{v:.5f}"


def show(path, class_name, P, r, predictors=False, reflections=False, cepstrum_q=None, from_=1, to=0):
    """-> (stdout, stderr, selected rows) of prd_show_rs; selected rows is what --pickle saves.  Q <= P gives the
    message only; from_ > to_ + 1 raises IndexError (the Rust slice panic)."""
    out = [f"# {path}\n"]
    err = []
    r = np.asarray(r, dtype=np.float64).reshape(-1, P + 1)
    if cepstrum_q is not None:
        if not P < cepstrum_q:
            err.append(f"cepstrum value={cepstrum_q} must be > prediction order={P}")
            return "".join(out), "".join(err), None
        to_ = cepstrum_q - 1 if to == 0 or to >= cepstrum_q else to
        f = features(r, cepstrum_q)
        for s, pe in zip(f["status"], f["pe"]):
            if s != 0:
                err.append(f"WARNING: lpca_r: res_lpca = {s}, err_pred = {float(pe)!r}\n")
        vec, name = f["c"], "c"
    else:
        to_ = P if to == 0 or to > P else to
        if predictors:
            vec, name = lpca_r(r)[3], "a"
        elif reflections:
            vec, name = lpca_r(r)[2], "k"
        else:
            vec, name = r, "r"
    if from_ > to_ + 1:
        raise IndexError(f"{from_}..={to_}")
    sel = [list(map(float, row[from_:to_ + 1])) for row in vec]
    out.append(f"# class_name='{class_name}', T={len(vec)} P={P}\n")
    out.append(",".join(f"{name}{i}" for i in range(from_, to_ + 1)) + "\n")
    for row in sel:
        out.append(", ".join(rust_value(v) for v in row) + "\n")
    return "".join(out), "".join(err), sel
