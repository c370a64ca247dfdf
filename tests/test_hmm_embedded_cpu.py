"""`hmm learn --embedded`, CPU side: the numpy restatement against the contract transcribed in plain loops,
against an exact Fraction sum over every admissible path of the chain, and (one unit) against a plain numpy forward-backward of
one sequence; the conservation laws of the counts; the statuses; EM on the planted streams; the refusals of the entry points
and the CLI that come before any HIP call; the exports and the usage text; the kernels' compiler metadata.  The GPU parity
tests are in test_gpu_hmm_embedded.py."""
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_embedded_cases as cases
from . import hmm_embedded_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXE = os.path.join(CSRC, "ecoz2")
NINF = float("-inf")
U = 2.0 ** -53
M = cases.M


def _err():
    return e.lib.e2vq_last_error().decode()


def _one(models, seq, units, optional=None, ls=0.0, one=R.estep_one):
    return R.estep(models, np.asarray(seq), [0, len(seq)], np.asarray(units), [0, len(units)], optional, ls, one=one)


def tolerances(T, L, Nmax):
    """(absolute bound of a count, absolute bound of ln P).  First order, every term non-negative, so relative errors add.
    One forward step rounds, per state, at most: 2 N - 1 times in the chain, N - 1 times in the unit mass it reads, once in
    the sum of two unit masses, once in e = sw pi, once in the product with e, once in the add, once in the emission product,
    <= 6 + 16 times in the global sum and once in the division by it: 3 N + 28 =: r bounds
    them, and bounds a backward step (chain 2 N - 1, R chain 2 N - 1 with e, the sum of two R, the add, the product and the
    division of u) as well.  A count term -- gamma, xi or m u -- lies behind at most T forward steps, the final sum Z with its
    division, T backward steps and three products of its own: (2 T + 2) r roundings, a relative error of (2 T + 2) r U to first
    order; times 2 for the second order.  Every term is <= 1, a cell sums at most T L of them (a class may own every unit),
    and fix2 moves a term by at most 2^-61: count_tol = T L ((4 T + 4) r U + 2^-61).  ln P is the logarithm of T + 1 factors,
    each with at most r roundings: a relative error of P of (T + 1) r U, doubled for the second order, plus two roundings of
    the host's logarithm and multiplication on |ln P| <= 40 T: lp_tol = (2 T + 2) r U + 160 T U.
    The worst errors observed over the cases below: 0.0006 of count_tol, 0.42 of lp_tol (the reference's own two
    logarithms of big integers are in that figure)."""
    r = 3 * Nmax + 28
    return T * L * ((4 * T + 4) * r * U + 2.0 ** -61), (2 * T + 2) * r * U + 160 * T * U


# ---- the restatement's two forms ----------------------------------------------------------------------------------------------------
SMALL = [
    ("plain", (3, 2, 3), [0, 1, 2], None, 6),
    ("first optional", (3, 2, 3), [0, 1, 2], [1, 0, 0], 5),
    ("last optional", (3, 2, 3), [0, 1, 2], [0, 0, 1], 5),
    ("middle optional", (2, 3, 2), [0, 1, 2], [0, 1, 0], 6),
    ("immediate repeat", (3, 2), [0, 0, 1], None, 6),
    ("T = the mandatory units", (3, 2, 3), [0, 1, 2], [1, 0, 0], 2),
    ("T = L", (2, 3, 1), [2, 1, 0], None, 3),
    ("one unit", (3,), [0], None, 6),
]


def _small(case, zeros=0.3):
    name, Ns, units, opt, T = case
    models = cases.small_models(seed=len(name), Ns=Ns, zeros=zeros)
    rng = np.random.default_rng(T + len(units))
    return models, rng.integers(0, M, T), units, opt


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_the_vectorised_form_is_the_transcription_bit_for_bit(case):
    models, seq, units, opt = _small(case)
    for ls in (0.0, -1.5):
        a, b = _one(models, seq, units, opt, ls), _one(models, seq, units, opt, ls, one=R.transcribe)
        assert a["status"].tolist() == b["status"].tolist() and a["log_prob"].tobytes() == b["log_prob"].tobytes()
        assert all(np.array_equal(x, y) for x, y in zip(a["acc"], b["acc"]))


def test_fix2_and_unfix_are_the_kernels():
    x = np.array([0.0, 1.0, 0.5, 2.0 ** -29, 2.0 ** -60, 2.0 ** -61, 3 * 2.0 ** -61, 0.3, 1.0 - 2.0 ** -53, 5e-324])
    hi, lo = R.fix2(x)
    assert hi.tolist()[:4] == [0, 1 << 29, 1 << 28, 1] and lo.tolist()[:4] == [0, 0, 0, 0]
    assert (hi[4], lo[4]) == (0, 1) and (hi[5], lo[5]) == (0, 0) and (hi[6], lo[6]) == (0, 2) and (hi[9], lo[9]) == (0, 0)  # (ties to even)
    for v, h, l in zip(x, hi, lo):
        assert abs(R.unfix(h, l) - v) <= 2.0 ** -61
    assert R.unfix(3, -1) == (3 * 2 ** 31 - 1) / 2.0 ** 60 and R.acc_words(5, 8) == int(e.lib.e2vq_hmm_acc_words(5, 8))


# ---- against the exact sum over every admissible path ----------------------------------------------------------------------------------
def _exact(models, seq, units, optional, ls):
    """Fractions: P = the sum of the weights of all admissible paths, and the expected counts per class -> (P, counts) with
    counts[k] = dict PI, AN, BN, BD of Fractions (already divided by P)"""
    L, T = len(units), len(seq)
    # the sets of the contract, restated here so that the reference shares nothing with the restatement
    opt = [bool(x) for x in optional] if optional is not None else [False] * L
    S0 = {0} | ({1} if opt[0] else set())
    F = {L - 1} | ({L - 2} if opt[L - 1] else set())
    skip = [l >= 2 and opt[l - 1] for l in range(L)]  # unit l may be entered from l - 2
    fr = lambda x: Fraction(float(x))
    sw = fr(math.exp(ls))
    states = [(l, j) for l in range(L) for j in range(len(models[units[l]][0]))]
    cnt = [dict(PI={}, AN={}, BN={}, BD={}) for _ in models]
    total = [Fraction(0)]

    def bump(d, key, w):
        d[key] = d.get(key, Fraction(0)) + w

    def walk(t, l, i, w, events):
        if w == 0:
            return
        if t == T - 1:
            if l in F:
                total[0] += w
                for kind, k, key in events:
                    bump(cnt[k][kind], key, w)
            return
        o = int(seq[t + 1])
        k = units[l]
        pi, A, B = models[k]
        for j in range(len(pi)):  # within the unit
            walk(t + 1, l, j, w * fr(A[i][j]) * fr(B[j][o]), events + [("AN", k, (i, j)), ("BN", k, (j, o)), ("BD", k, j)])
        for l2 in [l + 1] + ([l + 2] if l + 2 < L and skip[l + 2] else []):  # into a later unit, through its pi
            if l2 >= L:
                continue
            k2 = units[l2]
            pi2, _A2, B2 = models[k2]
            for j in range(len(pi2)):
                walk(t + 1, l2, j, w * sw * fr(pi2[j]) * fr(B2[j][o]), events + [("PI", k2, j), ("BN", k2, (j, o)), ("BD", k2, j)])

    o0 = int(seq[0])
    for l, j in states:
        if l in S0:
            k = units[l]
            walk(0, l, j, fr(models[k][0][j]) * fr(models[k][2][j][o0]), [("PI", k, j), ("BN", k, (j, o0)), ("BD", k, j)])
    P = total[0]
    if P > 0:
        for c in cnt:
            for d in c.values():
                for key in d:
                    d[key] = d[key] / P
    return P, cnt


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_counts_and_p_against_the_exact_sum_over_every_path(case):
    """the tolerances are `tolerances`' (derived there, with the worst error observed)"""
    models, seq, units, opt = _small(case, zeros=0.0)
    T, L = len(seq), len(units)
    count_tol, lp_tol = tolerances(T, L, max(len(m[0]) for m in models))
    for ls in (0.0, -1.5):
        got = _one(models, seq, units, opt, ls)
        P, cnt = _exact(models, seq, units, opt, ls)
        assert got["status"].tolist() == [0] and P > 0
        lnP = math.log(P.numerator) - math.log(P.denominator)
        assert abs(got["log_prob"][0] - lnP) <= lp_tol, (got["log_prob"][0], lnP)
        worst = 0.0
        for k, (pi, _A, _B) in enumerate(models):
            N = len(pi)
            d = R.decode(got["acc"][k], N, M)
            for j in range(N):
                worst = max(worst, abs(Fraction(d["PI"][j]) - cnt[k]["PI"].get(j, 0)), abs(Fraction(d["BD"][j]) - cnt[k]["BD"].get(j, 0)))
                worst = max(worst, abs(Fraction(d["AD"][j]) - sum(cnt[k]["AN"].get((j, x), 0) for x in range(N))))
                for i in range(N):
                    worst = max(worst, abs(Fraction(d["AN"][i, j]) - cnt[k]["AN"].get((i, j), 0)))
                for o in range(M):
                    worst = max(worst, abs(Fraction(d["BN"][j, o]) - cnt[k]["BN"].get((j, o), 0)))
            assert d["used"] == (1 if k in units else 0) and d["skipped"] == 0
        print(case[0], ls, "count error", float(worst) / count_tol, "of the bound; ln P error", abs(got["log_prob"][0] - lnP) / lp_tol)
        assert worst <= count_tol, (float(worst), count_tol)


# ---- one unit is the forward-backward of one sequence -------------------------------------------------------------------------------
def test_one_unit_gives_the_counts_of_a_plain_forward_backward_and_pi_sums_to_one():
    model = cases.small_models(seed=4, Ns=(4,), zeros=0.0)[0]
    pi, A, B = model
    rng = np.random.default_rng(6)
    seq = rng.integers(0, M, 40)
    T, N = len(seq), 4
    al = np.zeros((T, N))
    c = np.zeros(T)
    for t in range(T):
        x = pi * B[:, seq[0]] if t == 0 else (al[t - 1] @ A) * B[:, seq[t]]
        c[t] = x.sum()
        al[t] = x / c[t]
    be = np.ones((T, N))
    for t in range(T - 2, -1, -1):
        be[t] = A @ (B[:, seq[t + 1]] * be[t + 1]) / c[t + 1]
    g = al * be
    AN = sum(np.outer(al[t], B[:, seq[t + 1]] * be[t + 1] / c[t + 1]) * A for t in range(T - 1))
    BN = np.zeros((N, M))
    np.add.at(BN.T, seq, g)
    got = _one([model], seq, [0], None, -2.0)  # (the price plays no part: nothing is entered)
    d = R.decode(got["acc"][0], N, M)
    count_tol, lp_tol = tolerances(T, 1, N)
    assert abs(got["log_prob"][0] - np.log(c).sum()) <= lp_tol
    for name, want in (("PI", g[0]), ("AN", AN), ("AD", g[:-1].sum(axis=0)), ("BN", BN), ("BD", g.sum(axis=0))):
        assert np.abs(d[name] - want).max() <= count_tol, name
    assert abs(d["PI"].sum() - 1.0) <= count_tol
    new = R.mstep([model], got["acc"], 0.0)[0]
    assert np.abs(new[0] - g[0]).max() <= 2 * count_tol  # the M-step's pi is gamma_0: the PI sum is 1


# ---- conservation ---------------------------------------------------------------------------------------------------------------------
def test_the_state_occupancies_of_a_frame_sum_to_one_and_bd_sums_to_t():
    streams, transcripts, optionals = cases.planted_batch(fills=("some",), seeds=(20, 21))
    models = cases.blurred(cases.planted_models())
    for seq, units, opt in zip(streams, transcripts, optionals):
        T, L = len(seq), len(units)
        count_tol, _lp = tolerances(T, L, 3)
        got = _one(models, seq, units, opt, -1.0)
        assert got["status"].tolist() == [0]
        ds = [R.decode(got["acc"][k], len(models[k][0]), M) for k in range(4)]
        # BN[., o] summed over classes, states and the symbol's column = the number of frames that show the symbol:
        # sum over states of g_t = 1 at every t, frame by frame where a symbol occurs once, and in every column's total
        for o in range(M):
            col = sum(d["BN"][:, o].sum() for d in ds)
            assert abs(col - int((seq == o).sum())) <= count_tol, o
        assert abs(sum(d["BD"].sum() for d in ds) - T) <= count_tol
        # PI counts the start and every entry: on a path, one for each unit it visits.  Every path visits all mandatory units
        # and at most all L, so the expectation lies between the two counts
        visited = sum(d["PI"].sum() for d in ds)
        assert sum(1 for x in opt if not x) - count_tol <= visited <= L + count_tol
    # frame by frame on a stream whose symbols are all different
    models = cases.small_models(seed=9, Ns=(3, 2, 3), zeros=0.0)
    seq = np.arange(M)
    got = _one(models, seq, [0, 1, 2, 1], [0, 1, 0, 1], -0.5)
    ds = [R.decode(got["acc"][k], len(models[k][0]), M) for k in range(3)]
    for t in range(M):
        assert abs(sum(d["BN"][:, t].sum() for d in ds) - 1.0) <= tolerances(M, 4, 3)[0]


# ---- statuses ---------------------------------------------------------------------------------------------------------------------------
def test_statuses_and_a_skipped_stream_leaves_every_limb():
    models = cases.small_models()
    rng = np.random.default_rng(3)
    good = [rng.integers(0, M, n) for n in (20, 9)]
    tr = [np.array([0, 1, 2]), np.array([2, 2, 0, 1])]
    op = [np.array([0, 1, 0], np.uint8), np.array([1, 0, 0, 1], np.uint8)]
    base = R.estep(models, *cases.pack(good, tr, op), -1.0)
    assert base["status"].tolist() == [0, 0]
    short = rng.integers(0, M, 1)  # two mandatory units, one frame
    bad = good[0].copy()
    bad[7] = M
    got = R.estep(models, *cases.pack(good + [short, bad], tr + [tr[0], tr[0]], op + [op[0], op[0]]), -1.0)
    assert got["status"].tolist() == [0, 0, 1, 2] and got["log_prob"][2:].tolist() == [NINF, NINF]
    for k, (a, b) in enumerate(zip(got["acc"], base["acc"])):
        assert np.array_equal(a[:-1], b[:-1]) and a[-1] == b[-1] + 2, k  # (both skipped streams name every class)
    # T below the number of mandatory units, and exactly at it
    dense = cases.small_models(zeros=0.0)
    assert _one(dense, good[0][:1], [0, 1, 2], [0, 1, 0])["status"].tolist() == [1]
    assert _one(dense, good[0][:2], [0, 1, 2], [0, 1, 0])["status"].tolist() == [0]
    assert _one(models, [], [0], None)["status"].tolist() == [1]
    impossible = [(np.ones(1), np.ones((1, 1)), np.array([[1.0, 0.0]]))]
    # the first event in frame order decides: a symbol >= M behind an impossible frame does not count
    assert _one(impossible, [0, 1, 2], [0], None)["status"].tolist() == [1]  # (c_1 = 0 comes before the symbol 2 >= M)
    assert _one(impossible, [0, 2, 1], [0], None)["status"].tolist() == [2]


# ---- EM on the planted streams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["some", "all"])
def test_em_on_the_planted_streams(fill):
    """Start: the planted models mixed half-and-half with the uniform model of their own type (cases.blurred: B with the uniform
    row, pi and the rows of A with the uniform distribution over their support, which keeps the left-to-right zeros); epsilon =
    0.  From this start every trained state's most likely symbol is PEAKS' on the restatement: the start was not moved.
    The margin by which sum ln P may fall: exact EM never lowers it (Baum's inequality holds for any polynomial with
    non-negative coefficients in parameters that are re-estimated as normalised expected counts, which the weighted chain is);
    in doubles each of the two evaluations of ln P is off by at most `tolerances`' lp_tol a stream, and each re-estimated
    parameter by a relative (T_all L + 2) U from the limb sums and the division, which moves ln P by at most 3 T_all times that
    (a frame uses one emission and one transition or entry): margin = S 2 lp_tol + 3 T_all (T_all L + 2) U.  No fall was
    observed: over the six E-steps of both cases every step rose, by 0.3 at the least."""
    streams, transcripts, optionals = cases.planted_batch(fills=(fill,), seeds=(20, 21, 22))
    args = cases.pack(streams, transcripts, optionals)
    start = cases.blurred(cases.planted_models())
    models, hist = R.train(start, *args, -1.0, 0.0, -1e300, 6)
    T_all, L = int(args[1][-1]), max(len(u) for u in transcripts)
    margin = len(streams) * 2 * tolerances(max(len(s) for s in streams), L, 3)[1] + 3 * T_all * (T_all * L + 2) * U
    assert len(hist) == 6
    falls = [a - b for a, b in zip(hist, hist[1:])]
    print(fill, hist, "margin", margin, "worst fall", max(falls))
    assert max(falls) <= margin, (falls, margin)
    assert hist[-1] > hist[0]
    for k in range(3):
        pi, A, B = models[k]
        assert pi.tolist() == [1.0, 0.0, 0.0]  # (a single non-zero entry is re-estimated to exactly 1)
        assert (A[np.tril_indices(3, -1)] == 0.0).all() and A[0, 2] == 0.0 and (A[np.triu_indices(3)][[0, 1, 3, 4, 5]] > 0).all()
        assert B.argmax(axis=1).tolist() == cases.PEAKS[k], (k, B.argmax(axis=1))
        assert np.abs(A.sum(axis=1) - 1).max() < 1e-12 and np.abs(B.sum(axis=1) - 1).max() < 1e-12
    fpi, fA, fB = models[cases.FILLER]
    assert not np.array_equal(fB, start[cases.FILLER][2]) and set(np.argsort(fB[0])[-2:]) == {6, 7}  # the filler is re-estimated too
    assert fpi.tolist() == [1.0] and fA.tolist() == [[1.0]]


def test_the_floor_and_an_unnamed_class():
    streams, transcripts, optionals = cases.planted_batch(fills=("all",), seeds=(20,))
    args = cases.pack(streams, transcripts, optionals)
    extra = cases.small_models(seed=2, Ns=(6,))[0]
    start = cases.blurred(cases.planted_models()) + [extra]
    models, hist = R.train(start, *args, -1.0, 1e-3, 1e300, -1)
    assert len(hist) == 2  # val_auto stops the second E-step, which gets no M-step
    assert all(np.asarray(a).tobytes() == np.asarray(b, dtype=np.float64).tobytes() for a, b in zip(models[4], extra))
    assert min(float(m[2].min()) for m in models[:4]) >= 1e-3 * 0.99 and all(np.abs(m[2].sum(axis=1) - 1).max() < 1e-12 for m in models[:4])
    with pytest.raises(ValueError):
        R.train(start, streams[0][:3], [0, 3], *args[2:], -1.0)


# ---- refusals before the device -------------------------------------------------------------------------------------------------------
def _call(models, sym, offs, units, unit_offs, optional=None, ls=0.0, train=False):
    K = len(models)
    ms = [tuple(np.ascontiguousarray(x, dtype=np.float64) for x in m) for m in models]
    ns = (C.c_int * max(K, 1))(*[len(m[0]) for m in ms])
    ptr = lambda i: (C.c_void_p * max(K, 1))(*[m[i].ctypes.data for m in ms])
    sym = np.ascontiguousarray(sym, dtype=np.uint16)
    offs, unit_offs = np.ascontiguousarray(offs, dtype=np.int64), np.ascontiguousarray(unit_offs, dtype=np.int64)
    units = np.ascontiguousarray(units, dtype=np.int32)
    opt = None if optional is None else np.ascontiguousarray(optional, dtype=np.uint8)
    S = len(offs) - 1
    if train:
        hist, n = np.zeros(8), C.c_int(0)
        return e.lib.e2vq_hmm_train_embedded(0, K, ns, M, ptr(0), ptr(1), ptr(2), sym.ctypes.data, offs.ctypes.data, S, units.ctypes.data,
                                             unit_offs.ctypes.data, opt.ctypes.data if opt is not None else None, ls, 1e-5, 0.3, 2,
                                             hist.ctypes.data, 8, C.byref(n), 0)
    acc = [np.zeros(R.acc_words(len(m[0]), M), dtype=np.int64) for m in ms]
    accp = (C.c_void_p * max(K, 1))(*[a.ctypes.data for a in acc])
    lp, st = np.zeros(max(S, 1)), np.zeros(max(S, 1), dtype=np.int32)
    return e.lib.e2vq_hmm_embedded_estep(0, K, ns, M, ptr(0), ptr(1), ptr(2), sym.ctypes.data, offs.ctypes.data, S, units.ctypes.data,
                                         unit_offs.ctypes.data, opt.ctypes.data if opt is not None else None, ls, accp, lp.ctypes.data,
                                         st.ctypes.data, 0)


@pytest.mark.parametrize("train", [False, True])
def test_what_align_refuses_is_refused_and_so_is_a_seventeenth_slot(train, monkeypatch):
    who = "e2vq_hmm_train_embedded" if train else "e2vq_hmm_embedded_estep"
    models = cases.small_models()
    sym = np.zeros(10, np.uint16)
    for kw, msg in [
        (dict(units=[0, 1, 3], unit_offs=[0, 3]), f"{who}: stream 0, unit 2 names the class 3 outside [0, 3)"),
        (dict(units=[0, 1], unit_offs=[0, 0]), f"{who}: stream 0 has an empty transcript"),
        (dict(units=[0, 1, 2], unit_offs=[0, 3], optional=[0, 1, 1]), f"{who}: stream 0, units 1 and 2 are both optional"),
        (dict(units=[0], unit_offs=[0, 1], optional=[1]), f"{who}: stream 0: every unit of the transcript is optional"),
        (dict(units=[0], unit_offs=[0, 1], ls=0.5), f"{who}: ln_switch = 0.5"),
        (dict(units=[0], unit_offs=[0, 1], ls=NINF), f"{who}: ln_switch = -inf: a finite price"),
        (dict(units=[0], unit_offs=[0, 1], ls=float("nan")), f"{who}: ln_switch = nan"),
    ]:
        assert _call(models, sym, [0, 10], train=train, **kw) == 1 and msg in _err(), (msg, _err())
    wide, units, stream = cases.packing("64x17")
    assert _call(wide, stream, [0, len(stream)], units, [0, len(units)], train=train) == 1
    assert f"{who}: stream 0: the units take 17 wave-slots of 64 lanes (at most 16" in _err()
    negative = [(m[0], m[1], -m[2]) for m in models]
    assert _call(negative, sym, [0, 10], [0], [0, 1], train=train) == 1 and "HMM parameter" in _err()
    monkeypatch.setenv("ECOZ2_HMM_EMBED_A", "registers")
    assert _call(models, sym, [0, 10], [0], [0, 1], train=train) == 1 and "ECOZ2_HMM_EMBED_A=registers: lds or global" in _err()
    monkeypatch.setenv("ECOZ2_HMM_EMBED_A", "global")
    monkeypatch.setenv("ECOZ2_HMM_EMBED_AN", "lds")
    wide16, units, stream = cases.packing("64x16")  # the AN table of three 64-state classes takes 195 KB
    assert _call(wide16, stream, [0, len(stream)], units, [0, len(units)], train=train) == 1
    assert "A in global memory and the AN table in LDS take" in _err()


def test_the_file_form_and_the_cli_refuse_before_the_device(tmp_path):
    names = ["a", "b", "bg", "c"]
    pm = cases.planted_models()
    for c, m in zip(names, [pm[0], pm[1], pm[3], pm[2]]):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)
    e.formats.write_seq(str(tmp_path / "x.seq"), "_", M, np.zeros(40, np.uint16))
    (tmp_path / "x.csv").write_text("segment,class\n0,a\n1,c\n")
    (tmp_path / "bad.csv").write_text("segment,class\n0,a\n1,zebra\n")
    files = [str(tmp_path / "hmms" / f"{c}.hmm") for c in names]
    seq, lab = [str(tmp_path / "x.seq")], [str(tmp_path / "x.csv")]
    for kw, msg in [
        (dict(out_dir=tmp_path / "hmms"), "would overwrite an input model"),
        (dict(out_dir=tmp_path / "o", filler="wind"), "e2vq_hmm_learn_embedded_files: the filler 'wind' is no model's class"),
        (dict(out_dir=tmp_path / "o", ln_switch=1.0), "e2vq_hmm_learn_embedded_files: ln_switch = 1"),
        (dict(out_dir=tmp_path / "o", label_filenames=[str(tmp_path / "bad.csv")]), "bad.csv:3: 'zebra' is no model's class"),
        (dict(out_dir=tmp_path / "o", W_ms=0), "e2vq_hmm_learn_embedded_files: window 0 ms"),
    ]:
        args = dict(model_filenames=files, input_filenames=seq, label_filenames=lab)
        args.update(kw)
        with pytest.raises(Exception) as err:
            hmm.learn_embedded_files(**args)
        assert msg in str(err.value), (msg, str(err.value))
    assert not (tmp_path / "o").exists()
    with pytest.raises(ValueError):
        hmm.learn_embedded_files(files, seq, [], tmp_path / "o")
    run = lambda *a: subprocess.run([EXE, "hmm", "learn", "--embedded", *a], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    common = ["--models", "hmms", "--labels", "x.csv", "-o", "o", "--sequences", "x.seq"]
    for flag in (["--all-classes"], ["--grid"], ["--class-name", "a"]):
        r = run(*common, *flag)
        assert r.returncode == 2 and f"hmm learn --embedded excludes {flag[0]}" in r.stderr
    r = run("--models", "hmms", "--labels", "x.csv", "--sequences", "x.seq")
    assert r.returncode == 2 and "-o <dir> is required" in r.stderr
    r = run(*common, "--switch-penalty", "-inf")
    assert r.returncode == 2 and "finite and at most 0" in r.stderr
    r = run("--models", "hmms", "--labels", "x.csv", "-o", "hmms", "--sequences", "x.seq")
    assert r.returncode == 1 and "would overwrite an input model" in r.stdout
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert "ecoz2 hmm learn --embedded -m|--models" in r.stderr + r.stdout


def test_the_refusals_shared_with_the_other_transcript_commands_keep_every_word(tmp_path):
    """Byte for byte, with the name of the entry point and of the label file in front: the seventeenth slot with its closing
    words, from arrays and from files (17 units of one 64-state class), and a label file without a unit."""
    uni = lambda N, m: (np.full(N, 1.0 / N), np.full((N, N), 1.0 / N), np.full((N, m), 1.0 / m))
    slots = "stream 0: the units take 17 wave-slots of 64 lanes (at most 16: the embedded E-step has no looped body)"
    for train, who in ((False, "e2vq_hmm_embedded_estep"), (True, "e2vq_hmm_train_embedded")):
        assert _call([uni(64, M), uni(2, M)], np.zeros(8, np.uint16), [0, 8], [0] * 17, [0, 17], train=train) == 1
        assert _err() == f"{who}: {slots}"
    for c, N in (("a", 64), ("b", 2)):
        hmm.save_model(tmp_path / f"{c}.hmm", c, *uni(N, 4))
    e.formats.write_seq(str(tmp_path / "x.seq"), "_", 4, np.zeros(8, np.uint16))
    (tmp_path / "wide.csv").write_text("class\n" + "a\n" * 17)
    (tmp_path / "empty.csv").write_text("class\n")
    files = [str(tmp_path / "a.hmm"), str(tmp_path / "b.hmm")]
    for lab, msg in (("wide.csv", f"{tmp_path / 'wide.csv'}: e2vq_hmm_learn_embedded_files: {slots}"),
                     ("empty.csv", f"{tmp_path / 'empty.csv'}: no labelled units")):
        with pytest.raises(e.Ecoz2Error):
            hmm.learn_embedded_files(files, [str(tmp_path / "x.seq")], [str(tmp_path / lab)], tmp_path / "o")
        assert _err() == msg
    assert not (tmp_path / "o").exists()


def test_embedded_library_exports():
    for name in ("e2vq_hmm_embedded_estep", "e2vq_hmm_train_embedded", "e2vq_hmm_embedded_last_kernel_ms", "e2vq_hmm_learn_embedded_files"):
        assert hasattr(e.lib, name)
        assert name + "(" in open(os.path.join(ROOT, "include", "ecoz2_classify.h")).read()
    for fn in (hmm.embedded_estep, hmm.train_embedded, hmm.embedded_last_kernel_ms, hmm.learn_embedded_files):
        assert callable(fn)


def test_the_header_and_the_design_carry_the_same_contract():
    text = lambda s: re.sub(r"\s+", " ", re.sub(r"(?m)^ \*( |$)", "", s)).strip()
    header = open(os.path.join(ROOT, "include", "ecoz2_classify.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    h = text(header[header.index("`hmm learn --embedded`: re-estimate"):header.index("a larger stream alone.") + 22])
    d = text(design[design.index("`hmm learn --embedded`: re-estimate"):design.index("a larger stream alone.") + 22])
    assert h == d and len(h) > 4000


# ---- compiler metadata (read as test_hmm_posteriors_cpu.py reads its kernels') ------------------------------------------------------
VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_embed.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_embed.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _meta(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    return lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))


@pytest.mark.parametrize("pattern", [r"k_hmm_embed_fbILb0EE", r"k_hmm_embed_fbILb1EE", r"k_hmm_embed_rowsumE", r"k_hmm_reestimate_embeddedE",
                                     r"k_hmm_embed_adjustbE"])
def test_embedded_kernels_have_no_scratch_no_spill_and_fit_their_budget(asm, pattern):
    g = _meta(asm, pattern)
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
    print(pattern, "vgpr", g("vgpr_count"), "sgpr", g("sgpr_count"))
