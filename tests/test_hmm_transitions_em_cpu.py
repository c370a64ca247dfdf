"""`hmm transitions --em`, CPU side: the numpy restatement against the contract transcribed in plain loops,
against an exact Fraction sum of the expected bigram counts over every composite path, and against the sibling restatement
of 4.8.13 for ln P and the status; the exact zeros and the integer row sums; the rules of the M-step; EM on planted data (the
sum of ln P never falls, the planted grammar is recovered); the argument checks of the entry points, which run before any HIP
call; the CLI's refusals and its two usage lines; the exports; the written file read back; the kernel's compiler metadata.
The GPU parity tests are in test_gpu_hmm_transitions_em.py."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_trans_posterior_restatement as R13
from . import hmm_transitions_em_restatement as R
from .hmm_segment_trans_cases import random_model, random_prices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXE = os.path.join(CSRC, "ecoz2")
NINF = float("-inf")
U = 2.0 ** -53


def _err():
    return e.lib.e2vq_last_error().decode()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _uniform(N, M):
    return np.full(N, 1.0 / N), np.full((N, N), 1.0 / N), np.full((N, M), 1.0 / M)


def _models(kind, Ns, M, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return [random_model(rng, N, M) for N in Ns]
    if kind == "zeros":  # exact zeros in pi and A
        return [random_model(rng, N, M, 0.4) for N in Ns]
    return [_uniform(N, M) for N in Ns]


def _matrix(kind, K, seed=0):
    rng = np.random.default_rng(100 + seed)
    if kind == "random":
        return random_prices(rng, K)  # a 0.2 share -inf
    if kind == "never":
        return np.full((K, K), NINF)
    if kind == "free":
        return np.zeros((K, K))
    lt = -rng.uniform(0.0, 6.0, (K, K))
    if kind == "row":
        lt[K // 2, :] = NINF
    else:
        assert kind == "column"
        lt[:, K // 2] = NINF
    return lt


MATRICES = ["random", "never", "free", "row", "column"]


# ---- restatement == transcription ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "zeros", "uniform"])
@pytest.mark.parametrize("Ns", [(1,), (3,), (1, 1), (2, 3, 3, 1), (30, 30, 30), (64, 5), (1, 2) * 20])
def test_restatement_equals_the_transcription(kind, Ns):
    M, K = 5, len(Ns)
    models = _models(kind, Ns, M, 11)
    rng = np.random.default_rng(K)
    for T in (0, 1, 2, 7, 12 if max(Ns) > 8 else 40):
        seq = rng.integers(0, M, T)
        for mk in MATRICES:
            lt = _matrix(mk, K, T)
            a, b = R.new_acc(K), R.new_acc(K)
            got, want = R.estep_one(models, seq, lt, a), R.transcribe(models, seq, lt, b)
            assert got[1] == want[1] and _bits(got[0]) == _bits(want[0]), (T, mk)
            assert np.array_equal(a, b), (T, mk, np.argwhere(a != b)[:5])
            assert a[-2:].tolist() == [1, 0]
            if T < 2:
                assert not a[:-2].any()
    lt = _matrix("random", K)
    for bad in ([1, M, 2], [M]):
        a, b = R.new_acc(K), R.new_acc(K)
        assert R.estep_one(models, bad, lt, a) == R.transcribe(models, bad, lt, b) == (NINF, 2)
        assert np.array_equal(a, b) and not a[:-2].any() and a[-2:].tolist() == [0, 1]


def test_a_stream_the_loop_cannot_emit_adds_nothing_and_is_counted_as_skipped():
    pi, A, B = (x.copy() for x in _uniform(2, 3))
    B[:, 2] = 0.0
    for one in (R.estep_one, R.transcribe):
        acc = R.new_acc(1)
        assert one([(pi, A, B)], [0, 2, 1], [[-1.0]], acc) == (NINF, 1)
        assert acc.tolist() == [0, 0, 0, 1]


# ---- ln P and status: the bits of 4.8.13's restatement ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "zeros"])
@pytest.mark.parametrize("Ns", [(1,), (5,) * 13, (21, 22, 64), (3, 5, 4)])
def test_log_prob_and_status_are_the_sibling_restatements_bits(kind, Ns):
    M, K = 6, len(Ns)
    models = _models(kind, Ns, M, 23)
    rng = np.random.default_rng(K)
    lens = (0, 1, 2, 65, 130, 3)
    sym = rng.integers(0, M, sum(lens))
    sym[-2] = M  # the last stream: a symbol outside the alphabet
    offs = np.concatenate([[0], np.cumsum(lens)])
    for mk in MATRICES:
        lt = _matrix(mk, K, 1)
        got, want = R.estep(models, sym, offs, lt), R13.posteriors(models, sym, offs, lt)
        assert np.array_equal(got["status"], want["status"]) and got["status"].tolist() == [0] * 5 + [2], mk
        assert np.array_equal(_bits(got["log_prob"]), _bits(want["log_prob"])), mk
        assert got["acc"][-2:].tolist() == [5, 1]


# ---- brute force: an exact sum of the expected bigram counts over every composite path ------------------------------------
def _brute(models, seq, lt):
    """exact C[f][k] (Fractions) and P(O | loop).  One step from (f, i) to (k, j) weighs [f == k] A_f[i][j] + w[f][k] pi_k[j]; the
    second term is the succession f -> k, so a path of weight wt counts wt * (w[f][k] pi_k[j]) / (the step's weight) for it."""
    F = lambda x: Fraction(float(x))
    K, T = len(models), len(seq)
    w = [[F(math.exp(float(lt[f][k]))) for k in range(K)] for f in range(K)]
    states = [(k, j) for k, m in enumerate(models) for j in range(len(m[0]))]
    num = [[Fraction(0)] * K for _ in range(K)]
    total = Fraction(0)
    for path in itertools.product(states, repeat=T):
        k, j = path[0]
        wt = F(models[k][0][j]) * F(models[k][2][j][seq[0]])
        shares = []
        for t in range(1, T):
            k2, j2 = path[t]
            enter = w[k][k2] * F(models[k2][0][j2])
            step = enter + (F(models[k][1][j][j2]) if k2 == k else 0)
            wt *= step * F(models[k2][2][j2][seq[t]])
            if not wt:
                break
            shares.append((k, k2, enter / step))
            k, j = k2, j2
        if not wt:
            continue
        total += wt
        for f, k2, share in shares:
            num[f][k2] += wt * share
    return [[x / total for x in row] for row in num], total


BRUTE_MATRICES = {  # K = 3 (cut to the models' K): asymmetric with -inf entries; a row all -inf; a column all -inf
    "asymmetric": [[-0.5, NINF, -2.0], [-3.0, -0.25, NINF], [NINF, -1.0, -4.0]],
    "row": [[-1.0, -0.5, -2.0], [NINF, NINF, NINF], [-0.25, -3.0, -1.5]],
    "column": [[-1.0, NINF, -2.0], [-0.75, NINF, -0.5], [-0.25, NINF, -1.5]],
    "free": [[0.0] * 3] * 3,
}


def tolerance(T, Nmax, K):
    """Derived.  One xi_t[f][k] = S_t[f] * (w[f][k] * R_t[k]) is a product of a forward and a backward quantity of 4.8.13, so that
    section's first-order bound holds for it: every term is non-negative, relative errors add, 2 N + 2 K + 32 bounds a step
    (the two products that form xi lie within the 32), 2 T + 1 steps lie between a value and the parameters, the factor 4
    covers the second order; xi <= 1, so the relative bound is an absolute one.  A count sums T - 1 of them, each truncated by
    fix2 to a multiple of 2^-60 (half a unit: 2^-61), and the sum (<= T - 1) is rounded once by unfix."""
    per_xi = 4.0 * (2 * T + 1) * (2 * Nmax + 2 * K + 32) * U
    return (T - 1) * (per_xi + 2.0 ** -61) + (T - 1) * U


@pytest.mark.parametrize("kind", ["random", "zeros", "uniform"])
@pytest.mark.parametrize("Ns", [(1,), (2, 1), (2, 2), (1, 2, 2), (2, 2, 2)])
def test_brute_force_over_every_composite_path(kind, Ns):
    M, K = 3, len(Ns)
    models = _models(kind, Ns, M, 5)
    rng = np.random.default_rng(sum(Ns))
    worst = 0.0
    for T in (2, 3, 4, 5):
        if T == 5 and sum(Ns) > 5:  # (6^5 paths of Fractions a matrix: the five-frame sum stays with the smaller sets)
            continue
        seq = rng.integers(0, M, T)
        tol = tolerance(T, max(Ns), K)
        for name, full in BRUTE_MATRICES.items():
            lt = np.array(full)[:K, :K]
            acc = R.new_acc(K)
            lp, st = R.estep_one(models, seq, lt, acc)
            want, total = _brute(models, seq, lt)
            assert st == 0 and total > 0
            got = R.counts(acc, K)
            for f in range(K):
                for k in range(K):
                    err = abs(float(Fraction(float(got[f, k])) - want[f][k]))
                    worst = max(worst, err / tol)
                    assert err <= tol, (T, name, f, k, err, tol)
                    if lt[f, k] == NINF:  # a forbidden succession: no limb at all
                        assert acc[2 * (f * K + k)] == 0 and acc[2 * (f * K + k) + 1] == 0
            lnP = math.log(total.numerator) - math.log(total.denominator)
            assert abs(lp - lnP) <= tol + 4 * U * abs(lnP), (T, name)
    print(f"worst error / tolerance: {worst:.4f}")


# ---- exact zeros and row sums ------------------------------------------------------------------------------------------------
def test_all_prices_minus_infinity_give_every_limb_zero():
    models = _models("random", (3, 5, 4), 6, 2)
    sym = np.random.default_rng(1).integers(0, 6, 200)
    r = R.estep(models, sym, [0, 120, 200], np.full((3, 3), NINF))
    assert r["status"].tolist() == [0, 0] and not r["acc"][:-2].any() and r["acc"][-2:].tolist() == [2, 0]


def test_row_mass_is_the_integer_row_sum():
    K = 4
    models = _models("random", (3, 2, 5, 1), 6, 3)
    sym = np.random.default_rng(2).integers(0, 6, 300)
    acc = R.estep(models, sym, [0, 300], _matrix("random", K, 4))["acc"]
    for f in range(K):
        hi = sum(int(acc[2 * (f * K + k)]) for k in range(K))
        lo = sum(int(acc[2 * (f * K + k) + 1]) for k in range(K))
        D = R.row_mass(acc, K, f)
        assert Fraction(D) == Fraction(float(Fraction(hi * (1 << 31) + lo, 1 << 60)))  # the exact integer, rounded once
        assert abs(D - R.counts(acc, K)[f].sum()) <= 4 * K * U * D  # (the cells unfixed one by one round K times)
    # the mass that leaves the classes over a stream: one succession or none a step
    assert 0.0 < sum(R.row_mass(acc, K, f) for f in range(K)) <= 299.0


# ---- the M-step ------------------------------------------------------------------------------------------------------------
def test_mstep_rules():
    K = 3
    acc = R.new_acc(K)
    cell = lambda f, k, x: acc.__setitem__(slice(2 * (f * K + k), 2 * (f * K + k) + 2), [int(v) for v in R.fix2(x)])
    cell(0, 0, 1.5), cell(0, 1, 0.5), cell(0, 2, 2.0)   # row 0: counts 1.5, 0.5 and -- on a forbidden pair -- 2.0
    cell(2, 1, 3.0)                                     # row 2: one count; row 1: none
    ln_p = np.log(np.full((K, K), 1.0 / K))
    ln_p[0, 2] = NINF
    ln_p[1, 0] = NINF
    for alpha in (0.0, 1.0, 1e6):
        new = R.mstep(ln_p, acc, alpha)
        # a -inf entry stays whatever alpha; the counts that landed on it still belong to D[f]
        assert new[0, 2] == NINF and new[1, 0] == NINF
        den0 = 4.0 + alpha * 2.0
        assert new[0, 0] == math.log((1.5 + alpha) / den0) and new[0, 1] == math.log((0.5 + alpha) / den0)
        if alpha == 0.0:  # a row without mass keeps its bytes; an unseen pair of a row with mass becomes -inf
            assert np.array_equal(_bits(new[1]), _bits(ln_p[1]))
            assert new[2].tolist() == [NINF, 0.0, NINF]
        else:
            assert new[1, 1] == new[1, 2] == math.log((0.0 + alpha) / (0.0 + alpha * 2.0))
            assert new[2, 1] == math.log((3.0 + alpha) / (3.0 + alpha * 3.0))
        assert (new <= 0.0).all()
    rows = np.exp(R.mstep(ln_p, acc, 0.5)).sum(axis=1)
    assert abs(rows[1] - 1.0) <= 8 * U and abs(rows[2] - 1.0) <= 8 * U  # (row 0 holds mass on its forbidden pair)


# ---- EM on planted data ------------------------------------------------------------------------------------------------------
def planted(K=4, N=3, M=16, streams=4, frames=250, seed=7):
    """class models with well-separated emissions, and streams in which class k is followed by k + 1 (mod K) nine times in ten"""
    rng = np.random.default_rng(seed)
    models = []
    for k in range(K):
        pi = np.array([1.0] + [0.0] * (N - 1))
        A = np.zeros((N, N))
        for i in range(N):
            A[i, i], A[i, min(i + 1, N - 1)] = (0.7, 0.3) if i + 1 < N else (0.0, 1.0)
        B = np.full((N, M), 0.1 / (M - 2))
        for j in range(N):
            B[j, 4 * k + j], B[j, 4 * k + 3] = 0.7, 0.2
        models.append((pi, A, B / B.sum(axis=1, keepdims=True)))
    seqs = []
    for _ in range(streams):
        out, k = [], int(rng.integers(0, K))
        while len(out) < frames:
            pi, A, B = models[k]
            j = 0
            for _t in range(int(rng.integers(8, 14))):
                out.append(int(rng.choice(M, p=B[j])))
                j = int(rng.choice(N, p=A[j]))
            k = (k + 1) % K if rng.random() < 0.9 else int(rng.choice([c for c in range(K) if c != (k + 1) % K]))
        seqs.append(np.array(out[:frames], dtype=np.uint16))
    return models, seqs


def test_em_on_planted_data_never_lowers_the_likelihood_and_recovers_the_grammar():
    K = 4
    models, seqs = planted()
    sym, offs = hmm._pack(seqs)
    ln_p, hist = R.train(models, sym, offs, None, ln_switch=-2.0, alpha=0.0, val_auto=1e-4, max_iterations=12)
    print("sum ln P per E-step:", ["%.6f" % v for v in hist])
    assert len(hist) >= 3
    for a, b in zip(hist[:-1], hist[1:]):
        assert b - a >= -1e-9 * abs(a), (a, b)
    assert hist[-1] > hist[0]
    P = np.exp(ln_p)
    print(np.round(P, 3))
    assert [int(np.argmax(P[f])) for f in range(K)] == [(f + 1) % K for f in range(K)]
    assert np.max(np.abs(P.sum(axis=1) - 1.0)) <= 16 * U


# ---- e2vq_hmm_transitions_estep / e2vq_hmm_train_transitions: refusals before the device --------------------------------------
def _call_c(models, lt, Ns=None, K=None, acc=True, train=False, ln_switch=-1.0, alpha=1.0):
    Ns = [len(m[0]) for m in models] if Ns is None else Ns
    K = len(models) if K is None else K
    n = max(len(models), 1)
    ns = (C.c_int * n)(*Ns)
    keep = [[np.ascontiguousarray(m[i], dtype=np.float64) for m in models] for i in range(3)]
    ptr = lambda i: (C.c_void_p * n)(*[a.ctypes.data for a in keep[i]])
    sym, offs = np.zeros(8, np.uint16), np.array([0, 8], np.int64)
    lt = None if lt is None else np.ascontiguousarray(lt, dtype=np.float64)
    ltp = lt.ctypes.data if lt is not None else None
    a = np.zeros(2 * n * n + 2, dtype=np.int64)
    if train:
        return e.lib.e2vq_hmm_train_transitions(0, K, ns, 8, ptr(0), ptr(1), ptr(2), sym.ctypes.data, offs.ctypes.data, 1, ltp, ln_switch,
                                                alpha, 0.3, 2, None, 0, None, hmm.HMM_LEARN_CALLBACK(lambda _v, _x: None), 0)
    return e.lib.e2vq_hmm_transitions_estep(0, K, ns, 8, ptr(0), ptr(1), ptr(2), sym.ctypes.data, offs.ctypes.data, 1, ltp,
                                            a.ctypes.data if acc else None, None, None, 0)


def _bad(where, value):
    pi, A, B = (x.copy() for x in _uniform(3, 8))
    {"pi": pi, "A": A, "B": B}[where].flat[1] = value
    return pi, A, B


W = "e2vq_hmm_transitions_estep: "


@pytest.mark.parametrize("case,needle", [
    ("K0", W + "0 models (at least 1)"),
    ("no_lt", W + "bad arguments"),
    ("no_acc", W + "bad arguments"),
    ("N65", W + "model 0 has N=65 states (1 .. 64)"),
    ("lt_nan", W + "lt[1][0] = nan: the logarithm of a price, at most 0 (-inf forbids the succession)"),
    ("lt_pos", W + "lt[0][1] = 0.5: the logarithm of a price, at most 0"),
    ("slots17", W + "the classes take 17 wave-slots of 64 lanes (at most 16: the E-step of the class transitions has no looped body)"),
    ("slots17_packed", W + "the classes take 17 wave-slots of 64 lanes (at most 16"),
    ("negative", "HMM parameter A[1] = -0.25: not a finite non-negative number"),
    ("route", "ECOZ2_HMM_TRANS_EM_C=shared: lds or global"),
    ("forced_lds", W + "150 classes of 150 states with the count table in LDS take"),
])
def test_estep_refuses_before_the_device(case, needle, monkeypatch):
    ok = _uniform(3, 8)
    z = lambda K: np.full((K, K), -1.0)
    if case == "K0":
        rc = _call_c([ok], z(1), K=0)
    elif case == "no_lt":
        rc = _call_c([ok], None)
    elif case == "no_acc":
        rc = _call_c([ok], z(1), acc=False)
    elif case == "N65":
        rc = _call_c([_uniform(65, 8)], z(1))
    elif case == "lt_nan":
        rc = _call_c([ok, ok], [[0.0, -1.0], [float("nan"), -1.0]])
    elif case == "lt_pos":
        rc = _call_c([ok, ok], [[0.0, 0.5], [-1.0, -1.0]])
    elif case == "slots17":
        rc = _call_c([_uniform(64, 8)] * 17, z(17))
    elif case == "slots17_packed":
        rc = _call_c([_uniform(33, 8)] * 17, z(17))
    elif case == "negative":
        rc = _call_c([ok, _bad("A", -0.25)], z(2))
    elif case == "route":
        monkeypatch.setenv("ECOZ2_HMM_TRANS_EM_C", "shared")
        rc = _call_c([ok], z(1))
    else:
        monkeypatch.setenv("ECOZ2_HMM_TRANS_EM_C", "lds")
        rc = _call_c([_uniform(1, 8)] * 150, z(150))
    assert rc == 1 and needle in _err(), _err()


def test_train_refuses_before_the_device():
    ok, z = _uniform(3, 8), np.full((2, 2), -1.0)
    who = "e2vq_hmm_train_transitions: "
    assert _call_c([ok, ok], z, train=True, ln_switch=0.5) == 1 and who + "ln_switch = 0.5" in _err(), _err()
    assert _call_c([ok, ok], z, train=True, alpha=-1.0) == 1 and who + "alpha = -1: a finite number, at least 0" in _err(), _err()
    assert _call_c([ok, ok], z, train=True, alpha=float("nan")) == 1 and who + "alpha = nan" in _err(), _err()
    assert _call_c([_uniform(64, 8)] * 17, np.full((17, 17), -1.0), train=True) == 1 and who + "the classes take 17 wave-slots" in _err()
    assert e.lib.e2vq_hmm_transitions_acc_words(20) == 802 and hmm.transitions_acc_words(3) == 20 == R.acc_words(3)


def test_sixteen_slots_are_accepted_as_far_as_the_device():
    rc = _call_c([_uniform(64, 8)] * 16, np.full((16, 16), -1.0))
    if e.lib.e2vq_device_count() > 0:
        assert rc == 0, _err()
    else:
        assert rc == 1 and "no HIP device" in _err(), _err()


def test_python_mirror_raises_the_refusal():
    sym = np.zeros(8, np.uint16)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.transitions_estep([_uniform(3, 8)], sym, [0, 8], [[1.0]])
    assert "lt[0][0] = 1" in str(ei.value)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.train_transitions([_uniform(64, 8)] * 17, sym, [0, 8])
    assert "17 wave-slots" in str(ei.value)
    with pytest.raises(ValueError):
        hmm.transitions_estep([_uniform(3, 8)] * 2, sym, [0, 8], np.zeros((3, 3)))
    with pytest.raises(ValueError):
        hmm.transitions_estep([_uniform(3, 8)] * 2, sym, [0, 8], np.zeros((2, 2)), acc=np.zeros(9, dtype=np.int64))


# ---- the file form and the CLI ----------------------------------------------------------------------------------------------
@pytest.fixture
def corpus(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    models = []
    for c, N in (("A", 3), ("B", 5)):
        hmm.save_model(d / f"{c}.hmm", c, *_uniform(N, 16))
        models.append(str(d / f"{c}.hmm"))
    (d / "many").mkdir()
    for k in range(17):
        hmm.save_model(d / "many" / f"c{k:02d}.hmm", f"c{k:02d}", *_uniform(64, 16))
    e.formats.write_seq(str(d / "x.seq"), "A", 16, np.arange(40) % 16)
    (d / "t.csv").write_text("class,A,B\nA,0,-1\nB,-2,-inf\n")
    (d / "tpos.csv").write_text("class,A,B\nA,0,-1\nB,2,-inf\n")
    (d / "seg.csv").write_text("class\nA\nB\nA\n")
    return tmp_path, d, models


def test_files_refuse_before_the_device(corpus):
    tmp_path, d, models = corpus
    who = "e2vq_hmm_learn_transitions_files: "
    out, x = tmp_path / "out.csv", [str(d / "x.seq")]
    many = [str(d / "many" / f"c{k:02d}.hmm") for k in range(17)]

    def call(models, inputs, ls=-5.0, init=None, alpha=1.0, out=out):
        try:
            hmm.learn_transitions_files(models, inputs, out if out else "", ls, init=init, alpha=alpha, max_iterations=2)
        except e.Ecoz2Error as ex:
            return str(ex)
        return ""

    assert who + "the classes take 17 wave-slots of 64 lanes (at most 16: the E-step of the class transitions" in call(many, x)
    assert who + "no models" in call([], x)
    assert who + "no inputs" in call(models, [])
    assert who + "no output file" in call(models, x, out=None)
    assert who + "ln_switch = 2" in call(models, x, ls=2.0)
    assert who + "alpha = -0.5" in call(models, x, alpha=-0.5)
    assert "tpos.csv:3: B -> A = 2" in call(models, x, init=d / "tpos.csv")
    assert "nowhere.csv" in call(models, x, init=d / "nowhere.csv")
    assert not out.exists() and not (tmp_path / "out.csv.em.csv").exists()


def _cli(cwd, *args):
    r = subprocess.run([EXE, "hmm", "transitions", *args], cwd=cwd, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


MODELS = ["-m", "in/A.hmm", "in/B.hmm"]


@pytest.mark.parametrize("args,code,needle", [
    (["--em"] + MODELS + ["-o", "out.csv", "--sequences", "in/x.seq"], 2, "hmm transitions --em: --switch-penalty <x <= 0 | -inf> is required"),
    (["--em"] + MODELS + ["--switch-penalty", "1", "-o", "out.csv", "--sequences", "in/x.seq"], 2, "--switch-penalty 1: at most 0"),
    (["--em"] + MODELS + ["--switch-penalty", "-1", "--sequences", "in/x.seq"], 2, "hmm transitions --em: -o <file.csv> is required"),
    (["--em"] + MODELS + ["--switch-penalty", "-1", "-o", "out.csv", "--predictors", "in/x.prd"], 2, "need --codebook <cbook>"),
    (["--em"] + MODELS + ["--switch-penalty", "-1", "-o", "out.csv", "--alpha", "-1", "--sequences", "in/x.seq"], 2, "--alpha -1: at least 0"),
    (MODELS + ["-o", "out.csv", "--init", "in/t.csv", "in/seg.csv"], 2, "hmm transitions: --init needs --em"),
    (MODELS + ["-o", "out.csv", "-a", "0.1", "in/seg.csv"], 2, "hmm transitions: -a needs --em"),
    (MODELS + ["-o", "out.csv", "-I", "3", "in/seg.csv"], 2, "hmm transitions: -I needs --em"),
    (MODELS + ["-o", "out.csv", "--sequences", "in/x.seq"], 2, "hmm transitions: --sequences needs --em"),
    (MODELS + ["-o", "out.csv", "--predictors", "in/x.prd"], 2, "hmm transitions: --predictors needs --em"),
    (MODELS + ["-o", "out.csv", "--signals", "in/x.wav"], 2, "hmm transitions: --signals needs --em"),
    # past the flags: the library's refusals, exit status 1 on stdout
    (["--em"] + MODELS + ["--switch-penalty", "-1", "-o", "out.csv", "--init", "in/tpos.csv", "--sequences", "in/x.seq"], 1,
     "in/tpos.csv:3: B -> A = 2"),
    (["--em", "-m", "in/many", "--switch-penalty", "-1", "-o", "out.csv", "--sequences", "in/x.seq"], 1,
     "the classes take 17 wave-slots of 64 lanes"),
])
def test_cli_refusals(corpus, args, code, needle):
    tmp_path, _d, _models = corpus
    rc, out, err = _cli(tmp_path, *args)
    assert rc == code and needle in (err if code == 2 else out), (rc, out, err)
    assert not (tmp_path / "out.csv").exists()


def test_without_em_the_command_is_as_it_was(corpus):
    tmp_path, _d, _models = corpus
    rc, out, err = _cli(tmp_path, *MODELS, "--alpha", "1", "-o", "out.csv", "in/seg.csv")
    assert rc == 0 and err == "", (out, err)
    assert out == "1 inputs: 2 successions counted, 0 labels skipped (no model's class)\nout.csv saved (alpha 1, 2 classes)\n"
    want = [[math.log(1.0 / 3.0), math.log(2.0 / 3.0)], [math.log(2.0 / 3.0), math.log(1.0 / 3.0)]]
    assert np.array_equal(_bits(hmm.read_class_transitions(tmp_path / "out.csv", ["A", "B"])), _bits(want))


def test_usage_has_both_lines(tmp_path):
    rc, _out, err = _cli(tmp_path, "--em")
    assert rc == 2
    old = ("  ecoz2 hmm transitions -m|--models <files|dirs>... [--alpha 1] -o <file.csv> <segment .csv | selection table>...\n"
           "                  (the class-to-class prices for --class-transitions, from the successions of labelled segments)\n")
    new = ("  ecoz2 hmm transitions --em -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15] --switch-penalty <x>\n"
           "                  [--init <file.csv>] [--alpha 1] [-a val_auto] [-I max_iterations] -o <file.csv>\n"
           "                  --sequences <.seq>... | --predictors <.prd>... | --signals <.wav>...\n")
    assert old + new in err


def test_library_exports():
    names = ("e2vq_hmm_transitions_estep", "e2vq_hmm_transitions_acc_words", "e2vq_hmm_transitions_estep_last_kernel_ms",
             "e2vq_hmm_train_transitions", "e2vq_hmm_learn_transitions_files")
    header = open(os.path.join(ROOT, "include", "ecoz2_classify.h")).read()
    for name in names:
        assert hasattr(e.lib, name) and name + "(" in header
    for fn in ("transitions_estep", "transitions_estep_last_kernel_ms", "train_transitions", "learn_transitions_files"):
        assert callable(getattr(hmm, fn))


def test_an_m_step_result_round_trips_through_the_transitions_file(tmp_path):
    K = 3
    models = _models("random", (2, 3, 2), 6, 9)
    sym = np.random.default_rng(5).integers(0, 6, 150)
    start = np.log(np.full((K, K), 1.0 / K))
    start[1, 2] = NINF
    new = R.mstep(start, R.estep(models, sym, [0, 150], start - 1.0)["acc"], 0.25)
    names = ["rain", "ship", "whale"]
    hmm.write_class_transitions(tmp_path / "t.csv", names, new)
    back = hmm.read_class_transitions(tmp_path / "t.csv", names)
    assert np.array_equal(_bits(back), _bits(new)) and back[1, 2] == NINF and (back <= 0.0).all()


# ---- compiler metadata (read as test_hmm_trans_posteriors_cpu.py reads its kernels') --------------------------------------------
VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_trans_estep.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_trans_estep.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _meta(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    return lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))


@pytest.mark.parametrize("pattern", [r"k_hmm_trans_estepILb0ELb0EE", r"k_hmm_trans_estepILb0ELb1EE", r"k_hmm_trans_estepILb1ELb0EE",
                                     r"k_hmm_trans_estepILb1ELb1EE"])
def test_kernels_have_no_scratch_no_spill_and_fit_their_budget(asm, pattern):
    g = _meta(asm, pattern)
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
    print(pattern, "vgpr", g("vgpr_count"), "sgpr", g("sgpr_count"))
