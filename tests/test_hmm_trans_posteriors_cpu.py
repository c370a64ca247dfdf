"""`hmm segment --class-transitions --grammar-posteriors`, CPU side: the numpy restatement against the
contract transcribed in plain loops, against an exact Fraction sum over every composite path and against an np.longdouble
forward-backward over the one composite matrix -- at small class sets and at the rows of hmm_class_loop_cases.py that reach every
LDS layout of the kernel (K up to 1024), where the argmax also has to visit many classes --; the statuses and zero rows of the
event batch under every event set; the rows of post summing to 1; the two consequences of the contract (all
prices -inf: 4.8.7's bits at -inf; one finite price: 4.8.7's figures within the tolerance); the argument checks of
e2vq_hmm_segment_trans_posteriors and of the file form, which run before any HIP call; the CLI's new flag with its refusals;
the exports and the usage text; the kernel's compiler metadata.  The GPU parity tests are in
test_gpu_hmm_trans_posteriors.py."""
import ctypes as C
import inspect
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

from . import hmm_class_loop_cases as cases
from . import hmm_posterior_restatement as R7
from . import hmm_trans_posterior_restatement as R
from .hmm_segment_trans_cases import UNIFORM_PRICE, random_model, random_prices, uniform_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXE = os.path.join(CSRC, "ecoz2")
NINF = float("-inf")
U = 2.0 ** -53
LD = np.longdouble


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
    if kind == "uniform":
        return [_uniform(N, M) for N in Ns]
    hmm.set_random_seed(seed)
    return [hmm.init_model(N, M, 2 if kind == "cascade2" else 3) for N in Ns]


def _matrix(kind, K, seed=0):
    """the price matrices of the issue: asymmetric with -inf entries, a class that cannot be left, a class entered only at
    frame 0, and the two uniform ones"""
    rng = np.random.default_rng(100 + seed)
    if kind == "random":
        return random_prices(rng, K)
    if kind == "never":
        return np.full((K, K), NINF)
    if kind == "free":
        return np.zeros((K, K))
    if kind == "uniform":
        return np.full((K, K), UNIFORM_PRICE)
    lt = -rng.uniform(0.0, 6.0, (K, K))
    if kind == "row":
        lt[K // 2, :] = NINF
    else:
        assert kind == "column"
        lt[:, K // 2] = NINF
    return lt


MATRICES = ["random", "never", "free", "uniform", "row", "column"]


def tolerance(T, Nmax, K):
    """4.8.7's first-order argument (every term non-negative, so relative errors add) with what a step gains here: the class
    sum (<= N roundings), the walk over the K sources or targets (<= 2 K: a product and an add each) and the m * pi product;
    2 N + 2 K + 32 bounds a step, 2 T + 1 steps lie between a posterior and the parameters, the factor 4 covers the second
    order.  A posterior is at most 1, so the relative bound is an absolute one."""
    return 4.0 * (2 * T + 1) * (2 * Nmax + 2 * K + 32) * U


# ---- restatement == transcription ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "zeros", "uniform", "cascade2", "cascade3"])
@pytest.mark.parametrize("Ns", [(1,), (3,), (1, 1), (2, 3, 3, 1), (30, 30, 30), (64, 5), (1, 2) * 20])
def test_restatement_equals_the_transcription(kind, Ns):
    M, K = 5, len(Ns)
    models = _models(kind, Ns, M, 11)
    rng = np.random.default_rng(K)
    for T in (0, 1, 2, 7, 12 if max(Ns) > 8 else 40):
        seq = rng.integers(0, M, T)
        for mk in MATRICES:
            lt = _matrix(mk, K, T)
            got = R.posteriors_one(models, seq, lt)
            post, lp, st = R.transcribe(models, seq, lt)
            assert got["status"] == st and _bits(got["log_prob"]) == _bits(lp), (T, mk)
            assert got["post"].shape == (T, K) and np.array_equal(_bits(got["post"]), _bits(np.array(post).reshape(T, K))), (T, mk)
    lt = _matrix("random", K)
    got = R.posteriors_one(models, [1, M, 2], lt)
    assert (got["post"].tolist(), got["log_prob"], got["status"]) == R.transcribe(models, [1, M, 2], lt)
    assert got["status"] == 2 and got["log_prob"] == NINF and not got["post"].any()
    got = R.posteriors_one(models, [], lt)
    assert got["post"].shape == (0, K) and got["log_prob"] == 0.0 and got["status"] == 0


def test_a_stream_the_loop_cannot_emit_has_status_1():
    pi, A, B = (x.copy() for x in _uniform(2, 3))
    B[:, 2] = 0.0
    got = R.posteriors_one([(pi, A, B)], [0, 2, 1], [[-1.0]])
    assert got["status"] == 1 and got["log_prob"] == NINF and not got["post"].any()
    assert R.transcribe([(pi, A, B)], [0, 2, 1], [[-1.0]])[1:] == (NINF, 1)


# ---- brute force: an exact sum over every composite path ------------------------------------------------------------------
def _brute(models, seq, lt):
    """exact post (T x K Fractions) and P(O | loop): the sum over every path of composite states of pi B prod (W B), where
    one step from (f, i) to (k, j) weighs [f == k] A_f[i][j] + w[f][k] pi_k[j]"""
    F = lambda x: Fraction(float(x))
    K, T = len(models), len(seq)
    w = [[F(math.exp(float(lt[f][k]))) for k in range(K)] for f in range(K)]
    states = [(k, j) for k, m in enumerate(models) for j in range(len(m[0]))]
    num = [[Fraction(0)] * K for _ in range(T)]
    total = Fraction(0)
    for path in itertools.product(states, repeat=T):
        k, j = path[0]
        wt = F(models[k][0][j]) * F(models[k][2][j][seq[0]])
        for t in range(1, T):
            k2, j2 = path[t]
            step = w[k][k2] * F(models[k2][0][j2])
            if k2 == k:
                step += F(models[k][1][j][j2])
            wt *= step * F(models[k2][2][j2][seq[t]])
            k, j = k2, j2
            if not wt:
                break
        if not wt:
            continue
        total += wt
        for t in range(T):
            num[t][path[t][0]] += wt
    return [[x / total for x in row] for row in num], total


BRUTE_MATRICES = {  # K = 3 (cut to the models' K): asymmetric with -inf entries; a row all -inf; a column all -inf
    "asymmetric": [[-0.5, NINF, -2.0], [-3.0, -0.25, NINF], [NINF, -1.0, -4.0]],
    "row": [[-1.0, -0.5, -2.0], [NINF, NINF, NINF], [-0.25, -3.0, -1.5]],
    "column": [[-1.0, NINF, -2.0], [-0.75, NINF, -0.5], [-0.25, NINF, -1.5]],
    "never": [[NINF] * 3] * 3,
    "free": [[0.0] * 3] * 3,
}


@pytest.mark.parametrize("kind", ["random", "zeros", "uniform"])
@pytest.mark.parametrize("Ns", [(1,), (2, 1), (2, 2), (1, 2, 2), (2, 2, 2)])
def test_brute_force_over_every_composite_path(kind, Ns):
    M, K = 3, len(Ns)
    models = _models(kind, Ns, M, 5)
    rng = np.random.default_rng(sum(Ns))
    worst = 0.0
    for T in (1, 2, 3, 4, 5):
        if T == 5 and sum(Ns) > 5:  # (6^5 paths of Fractions a matrix: the five-frame sum stays with the smaller sets)
            continue
        seq = rng.integers(0, M, T)
        tol = tolerance(T, max(Ns), K)
        for name, full in BRUTE_MATRICES.items():
            lt = np.array(full)[:K, :K]
            r = R.posteriors_one(models, seq, lt)
            want, total = _brute(models, seq, lt)
            assert r["status"] == 0 and total > 0
            for t in range(T):
                for k in range(K):
                    err = abs(float(Fraction(float(r["post"][t, k])) - want[t][k]))
                    worst = max(worst, err / tol)
                    assert err <= tol, (T, name, t, k, err, tol)
            lnP = math.log(total.numerator) - math.log(total.denominator)
            assert abs(r["log_prob"] - lnP) <= tol + 4 * U * abs(lnP), (T, name)
    print(f"worst error / tolerance: {worst:.4f}")


# ---- extended precision: an independent forward-backward over the one composite matrix ------------------------------------
def _longdouble(models, seq, lt):
    Ns = [len(m[0]) for m in models]
    K, n = len(Ns), sum(Ns)
    at = np.concatenate([[0], np.cumsum(Ns)])
    cls = np.repeat(np.arange(K), Ns)
    pi = np.concatenate([np.asarray(m[0], dtype=LD) for m in models])
    B = np.concatenate([np.asarray(m[2], dtype=LD) for m in models])
    w = np.array([[math.exp(float(v)) for v in row] for row in np.asarray(lt)], dtype=LD)
    W = w[cls][:, cls] * pi[None, :]
    for k, m in enumerate(models):
        W[at[k]:at[k + 1], at[k]:at[k + 1]] += np.asarray(m[1], dtype=LD)
    T = len(seq)
    alpha, scale = np.zeros((T, n), dtype=LD), np.zeros(T, dtype=LD)
    for t in range(T):
        x = (pi if t == 0 else alpha[t - 1] @ W) * B[:, seq[t]]
        scale[t] = x.sum()
        alpha[t] = x / scale[t]
    beta = np.ones(n, dtype=LD)
    post = np.zeros((T, K), dtype=LD)
    for t in range(T - 1, -1, -1):
        g = alpha[t] * beta
        g = g / g.sum()
        post[t] = [g[at[k]:at[k + 1]].sum() for k in range(K)]
        if t > 0:
            beta = W @ (B[:, seq[t]] * beta)
            beta = beta / beta.sum()
    return post, np.log(scale).sum()


# (name) -> (Ns, M, T, matrix): positive models; computed once and shared by the two tests below
LONG_CASES = {
    "5x20_T1500_random": ([5] * 20, 16, 1500, "random"),
    "21_22_7_T200_row": ([21, 22, 7], 8, 200, "row"),
    "64_36_T300_column": ([64, 36], 4, 300, "column"),
    "3x5_T400_free": ([3] * 5, 6, 400, "free"),
    "33x3_T300_uniform": ([33] * 3, 8, 300, "uniform"),
}
_long_cache = {}


def _long(name):
    if name not in _long_cache:
        Ns, M, T, mk = LONG_CASES[name]
        models = _models("random", Ns, M, 17)
        seq = np.random.default_rng(T).integers(0, M, T)
        lt = _matrix(mk, len(Ns), 3)
        _long_cache[name] = (models, seq, lt, R.posteriors_one(models, seq, lt))
    return _long_cache[name]


@pytest.mark.parametrize("name", list(LONG_CASES))
def test_extended_precision_forward_backward(name):
    models, seq, lt, r = _long(name)
    Ns, T = LONG_CASES[name][0], len(seq)
    want, lnP = _longdouble(models, seq, lt)
    assert r["status"] == 0
    err = float(np.max(np.abs(r["post"].astype(LD) - want)))
    tol = tolerance(T, max(Ns), len(Ns))
    print(f"{name}: worst error {err:.3e}, tolerance {tol:.3e}, share {err / tol:.4f}")
    assert err <= tol
    assert abs(r["log_prob"] - float(lnP)) <= tol + 4 * U * abs(float(lnP))


@pytest.mark.parametrize("name", list(LONG_CASES))
def test_rows_sum_to_one(name):
    _m, seq, _lt, r = _long(name)
    Ns, T = LONG_CASES[name][0], len(seq)
    err = float(np.max(np.abs(r["post"].sum(axis=1) - 1.0)))
    print(f"{name}: rows sum to 1 within {err:.3e}")
    assert err <= tolerance(T, max(Ns), len(Ns))
    assert r["post"].min() >= 0.0


# ---- the rows, event sets and -inf rows that test_gpu_hmm_trans_posteriors_shapes.py runs (hmm_class_loop_cases.py) ---------
@pytest.mark.parametrize("name", list(cases.TRANS_POSTERIORS_SHAPES))
def test_the_restatement_at_the_layout_rows_against_extended_precision(name):
    """K up to 1024 and sum N up to 1024, where the restatement had been compared with nothing above K = 20"""
    models, stream, lt = cases.trans_posteriors_shape(name)
    Ns, T, K = cases.TRANS_POSTERIORS_SHAPES[name][0], len(stream), len(models)
    r = cases.trans_posteriors_reference(name)
    assert r["status"].tolist() == [0] and r["post"].shape == (T, K) and T == 130
    want, lnP = _longdouble(models, stream, lt)
    err = float(np.max(np.abs(r["post"].astype(LD) - want)))
    tol = tolerance(T, max(Ns), K)
    dlp = abs(float(r["log_prob"][0]) - float(lnP))
    visited = len(np.unique(r["post"].argmax(axis=1)))
    print(f"{name}: worst error {err:.3e}, tolerance {tol:.3e}, share {err / tol:.2e}, |ln P| differs by {dlp:.2e}, "
          f"the argmax visits {visited} classes")
    assert err <= tol
    assert dlp <= tol + 4 * U * abs(float(lnP))
    assert float(np.max(np.abs(r["post"].sum(axis=1) - 1.0))) <= tol and r["post"].min() >= 0.0
    if K >= 90:  # a wide row whose posterior sat on a few classes would not show a wrong walk over the others
        assert visited >= 10


@pytest.mark.parametrize("name", cases.TRANS_POSTERIORS_EVENT_SETS)
def test_the_restatement_on_the_event_batch_under_every_event_set(name):
    streams, kinds = cases.event_batch()
    T, S = cases.EVENT_T, len(streams)
    r = cases.trans_posteriors_event_reference(name)
    # (the first event in frame order decides: (DEAD, M) is 1, (M, DEAD) is 2)
    assert r["status"].tolist() == [0] + [2] * 6 + [1] * 6 + [1, 2] * 3 == [cases.event_status(k, "trans_posteriors") for k in kinds]
    assert np.isfinite(r["log_prob"][0]) and (r["log_prob"][1:] == NINF).all()
    failed = r["post"][T:]
    assert failed.shape == ((S - 1) * T, len(cases.EVENT_NS[name])) and not failed.any() and not np.signbit(failed).any()
    assert float(np.max(np.abs(r["post"][:T].sum(axis=1) - 1.0))) <= tolerance(T, max(cases.EVENT_NS[name]), failed.shape[1])


@pytest.mark.parametrize("name", ["64x3", "64x6_1x84"])
def test_all_prices_minus_infinity_are_the_single_price_bits_above_64_kb(name):
    models, stream, _lt = cases.trans_posteriors_shape(name)
    K, T = len(models), len(stream)
    got = R.posteriors(models, stream, [0, T], np.full((K, K), NINF))
    want = R7.posteriors(models, stream, [0, T], NINF)
    assert got["status"].tolist() == want["status"].tolist() == [0]
    assert np.array_equal(_bits(got["post"]), _bits(want["post"])) and np.array_equal(_bits(got["log_prob"]), _bits(want["log_prob"]))


# ---- the two consequences of the contract ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "zeros", "cascade3"])
@pytest.mark.parametrize("Ns", [(1,), (5,) * 13, (21, 22, 64), (3, 5, 4)])
def test_all_prices_minus_infinity_are_the_single_price_bits(kind, Ns):
    M, K = 6, len(Ns)
    models = _models(kind, Ns, M, 23)
    rng = np.random.default_rng(K)
    lens = (0, 1, 2, 65, 130)
    sym = rng.integers(0, M, sum(lens))
    offs = np.concatenate([[0], np.cumsum(lens)])
    got = R.posteriors(models, sym, offs, np.full((K, K), NINF))
    want = R7.posteriors(models, sym, offs, NINF)
    assert np.array_equal(got["status"], want["status"])
    assert np.array_equal(_bits(got["post"]), _bits(want["post"])) and np.array_equal(_bits(got["log_prob"]), _bits(want["log_prob"]))


@pytest.mark.parametrize("case", range(len(uniform_cases())))
def test_one_finite_price_gives_the_single_price_figures(case):
    name, models, streams = uniform_cases()[case]
    K, Nmax = len(models), max(len(m[0]) for m in models)
    lt = np.full((K, K), UNIFORM_PRICE)
    for seq in streams:
        got, want = R.posteriors_one(models, seq, lt), R7.posteriors_one(models, seq, UNIFORM_PRICE)
        tol = tolerance(len(seq), Nmax, K)
        assert got["status"] == want["status"] == 0, name
        err = float(np.max(np.abs(got["post"] - want["post"])))
        print(f"{name} T={len(seq)}: differs by {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol
        assert abs(got["log_prob"] - want["log_prob"]) <= tol + 4 * U * abs(want["log_prob"])


# ---- e2vq_hmm_segment_trans_posteriors: refusals before the device --------------------------------------------------------
def _call_c(models, lt, Ns=None, K=None):
    Ns = [len(m[0]) for m in models] if Ns is None else Ns
    K = len(models) if K is None else K
    n = max(len(models), 1)
    ns = (C.c_int * n)(*Ns)
    keep = [[np.ascontiguousarray(m[i], dtype=np.float64) for m in models] for i in range(3)]
    ptr = lambda i: (C.c_void_p * n)(*[a.ctypes.data for a in keep[i]])
    sym, offs = np.zeros(8, np.uint16), np.array([0, 8], np.int64)
    lt = None if lt is None else np.ascontiguousarray(lt, dtype=np.float64)
    return e.lib.e2vq_hmm_segment_trans_posteriors(0, K, ns, 8, ptr(0), ptr(1), ptr(2), sym.ctypes.data, offs.ctypes.data, 1,
                                                   lt.ctypes.data if lt is not None else None, None, None, None, 0)


def _bad(where, value):
    pi, A, B = (x.copy() for x in _uniform(3, 8))
    {"pi": pi, "A": A, "B": B}[where].flat[1] = value
    return pi, A, B


W = "e2vq_hmm_segment_trans_posteriors: "


@pytest.mark.parametrize("case,needle", [
    ("K0", W + "0 models (at least 1)"),
    ("no_lt", W + "bad arguments"),
    ("N0", W + "model 1 has N=0 states (1 .. 64)"),
    ("N65", W + "model 0 has N=65 states (1 .. 64)"),
    ("sumN", W + "4160 states in all models (at most 4096)"),
    ("lt_nan", W + "lt[1][0] = nan: the logarithm of a price, at most 0 (-inf forbids the succession)"),
    ("lt_pos", W + "lt[0][1] = 0.5: the logarithm of a price, at most 0"),
    ("slots17", W + "the classes take 17 wave-slots of 64 lanes (at most 16: the posteriors under class-to-class prices have no looped body)"),
    ("slots17_packed", W + "the classes take 17 wave-slots of 64 lanes (at most 16"),
    ("negative", "HMM parameter A[1] = -0.25: not a finite non-negative number"),
    ("nan", "HMM parameter pi[1] = nan: not a finite non-negative number"),
    ("inf", "HMM parameter B[1] = inf: not a finite non-negative number"),
])
def test_refuses_before_the_device(case, needle, monkeypatch):
    monkeypatch.setenv("ECOZ2_HMM_POSTERIOR_BODY", "looped")  # (not read here: there is one body)
    ok = _uniform(3, 8)
    z = lambda K: np.full((K, K), -1.0)
    if case == "K0":
        rc = _call_c([ok], z(1), K=0)
    elif case == "no_lt":
        rc = _call_c([ok], None)
    elif case == "N0":
        rc = _call_c([ok, ok], z(2), Ns=[3, 0])
    elif case == "N65":
        rc = _call_c([_uniform(65, 8)], z(1))
    elif case == "sumN":
        rc = _call_c([_uniform(64, 8)] * 65, z(65))
    elif case == "lt_nan":
        rc = _call_c([ok, ok], [[0.0, -1.0], [float("nan"), -1.0]])
    elif case == "lt_pos":
        rc = _call_c([ok, ok], [[0.0, 0.5], [-1.0, -1.0]])
    elif case == "slots17":
        rc = _call_c([_uniform(64, 8)] * 17, z(17))
    elif case == "slots17_packed":
        rc = _call_c([_uniform(33, 8)] * 17, z(17))  # (two classes of 33 do not share a slot)
    elif case == "negative":
        rc = _call_c([ok, _bad("A", -0.25)], z(2))
    elif case == "nan":
        rc = _call_c([_bad("pi", float("nan"))], z(1))
    else:
        rc = _call_c([_bad("B", float("inf"))], z(1))
    assert rc == 1 and needle in _err(), _err()


def test_sixteen_slots_are_accepted_as_far_as_the_device():
    rc = _call_c([_uniform(64, 8)] * 16, np.full((16, 16), -1.0))
    if e.lib.e2vq_device_count() > 0:
        assert rc == 0, _err()
    else:
        assert rc == 1 and "no HIP device" in _err(), _err()


def test_python_mirror_raises_the_refusal():
    sym = np.zeros(8, np.uint16)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment_trans_posteriors([_uniform(3, 8)], sym, [0, 8], [[1.0]])
    assert "lt[0][0] = 1" in str(ei.value)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment_trans_posteriors([_uniform(64, 8)] * 17, sym, [0, 8], np.zeros((17, 17)))
    assert "17 wave-slots" in str(ei.value)
    with pytest.raises(ValueError):
        hmm.segment_trans_posteriors([_uniform(3, 8)] * 2, sym, [0, 8], np.zeros((3, 3)))
    with pytest.raises(ValueError):
        hmm.segment_files(["a.hmm"], ["x.seq"], -1.0, grammar_posteriors=True)
    with pytest.raises(ValueError):  # (as before)
        hmm.segment_files(["a.hmm"], ["x.seq"], -1.0, class_transitions="t.csv", posteriors=True)
    with pytest.raises(ValueError):
        hmm.segment_files(["a.hmm"], ["x.seq"], -1.0, class_transitions="t.csv", grammar_posteriors=True, continuous="rec")
    with pytest.raises(ValueError):  # (as before)
        hmm.segment_files(["a.hmm"], ["x.seq"], -1.0, class_transitions="t.csv", frame_posteriors="frames")


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
    (d / "sub").mkdir()
    e.formats.write_seq(str(d / "sub" / "x.seq"), "A", 16, np.arange(40) % 16)
    (d / "t.csv").write_text("class,A,B\nA,0,-1\nB,-2,-inf\n")
    (d / "tpos.csv").write_text("class,A,B\nA,0,-1\nB,2,-inf\n")
    return tmp_path, d, models


def _files(models, inputs, transitions, ls=-5.0, csv=None, frames=None):
    m, _k1 = hmm._strs(models)
    f, _k2 = hmm._strs(inputs)
    return e.lib.e2vq_hmm_segment_trans_files_posteriors(m, len(models), None, f, len(inputs), 4, 45, 15, ls,
                                                         str(transitions).encode() if transitions else None,
                                                         str(csv).encode() if csv else None, str(frames).encode() if frames else None)


def test_files_refuse_before_the_device(corpus):
    tmp_path, d, models = corpus
    who = "e2vq_hmm_segment_trans_files_posteriors: "
    out, x = tmp_path / "out", [str(d / "x.seq")]
    many = [str(d / "many" / f"c{k:02d}.hmm") for k in range(17)]
    assert _files(many, x, d / "t.csv", csv=out, frames=out) == 1 and who + "the classes take 17 wave-slots" in _err(), _err()
    assert _files([], x, d / "t.csv", csv=out) == 1 and who + "no models" in _err()
    assert _files(models, x, None, csv=out) == 1 and who + "no class-transitions file" in _err()
    assert _files(models, x, d / "t.csv", ls=2.0, csv=out) == 1 and who + "ln_switch = 2" in _err()
    assert _files(models, x, d / "tpos.csv", csv=out) == 1 and "tpos.csv:3: B -> A = 2" in _err()
    assert _files(models, x + [str(d / "sub" / "x.seq")], d / "t.csv", frames=out) == 1 and "would both write" in _err(), _err()
    assert not out.exists()


def _cli(cwd, *args):
    r = subprocess.run([EXE, "hmm", "segment", *args], cwd=cwd, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


COMMON = ["--models", "in/A.hmm", "in/B.hmm", "--sequences", "in/x.seq", "--switch-penalty", "-5"]


@pytest.mark.parametrize("args,code,needle", [
    (COMMON + ["--grammar-posteriors"], 2, "hmm segment: --grammar-posteriors needs --class-transitions <file.csv>"),
    (COMMON + ["--grammar-posteriors", "--frame-posteriors", "frames"], 2, "hmm segment: --grammar-posteriors needs --class-transitions"),
    (COMMON + ["--class-transitions", "in/t.csv", "--grammar-posteriors", "--continuous", "rec"], 2,
     "hmm segment: --grammar-posteriors has the resident body and whole recordings only: not with --continuous or --body"),
    (COMMON + ["--class-transitions", "in/t.csv", "--grammar-posteriors", "--body", "looped"], 2,
     "hmm segment: --grammar-posteriors has the resident body and whole recordings only: not with --continuous or --body"),
    # the spelling with --posteriors stays refused as it was, with or without the new flag
    (COMMON + ["--class-transitions", "in/t.csv", "--posteriors"], 2,
     "hmm segment: --class-transitions and --posteriors exclude one another (the posteriors know one price only)"),
    (COMMON + ["--class-transitions", "in/t.csv", "--posteriors", "--grammar-posteriors"], 2,
     "hmm segment: --class-transitions and --posteriors exclude one another (the posteriors know one price only)"),
    # --frame-posteriors without either flag: the text it had
    (COMMON + ["--class-transitions", "in/t.csv", "--frame-posteriors", "frames"], 2,
     "hmm segment: --frame-posteriors <dir> needs --posteriors"),
    (COMMON + ["--class-transitions", "in/t.csv", "--grammar-posteriors", "--frame-posteriors"], 2, "--frame-posteriors needs a value"),
    # past the flags: the library's refusals, exit status 1 on stdout
    (COMMON[:6] + ["0", "--class-transitions", "in/tpos.csv", "--grammar-posteriors", "-c", "out"], 1, "in/tpos.csv:3: B -> A = 2"),
    (["--models", "in/many", "--sequences", "in/x.seq", "--switch-penalty", "-1", "--class-transitions", "in/t.csv",
      "--grammar-posteriors", "-c", "out", "--frame-posteriors", "frames"], 1, "the classes take 17 wave-slots of 64 lanes"),
])
def test_cli_refusals(corpus, args, code, needle):
    tmp_path, _d, _models = corpus
    rc, out, err = _cli(tmp_path, *args)
    assert rc == code and needle in (err if code == 2 else out), (rc, out, err)
    assert not (tmp_path / "out").exists() and not (tmp_path / "frames").exists()


def test_usage_names_the_flag_and_keeps_its_lines(tmp_path):
    rc, _out, err = _cli(tmp_path)
    assert rc == 2
    assert "                  [--class-transitions <file.csv>]\n                  [--grammar-posteriors [--frame-posteriors <dir>]]\n" in err
    assert "                  (--grammar-posteriors, with --class-transitions: the posteriors under those prices, reported as\n" in err
    for line in ("                  --switch-penalty <x <= 0 | -inf> [-c <csv dir|file.csv>]\n",
                 "                  [--posteriors [--frame-posteriors <dir>]]\n                  [--body <auto|resident|looped>]\n",
                 "                  [--continuous <name>]\n",
                 "                  (--class-transitions adds the file's price of every class-to-class succession to the penalty)\n"):
        assert line in err


def test_library_exports():
    for name in ("e2vq_hmm_segment_trans_posteriors", "e2vq_hmm_segment_trans_posteriors_last_kernel_ms",
                 "e2vq_hmm_segment_trans_files_posteriors"):
        assert hasattr(e.lib, name)
    assert callable(hmm.segment_trans_posteriors) and callable(hmm.segment_trans_posteriors_last_kernel_ms)
    params = inspect.signature(hmm.segment_files).parameters
    assert params["grammar_posteriors"].default is False and params["posteriors"].default is False
    header = open(os.path.join(ROOT, "include", "ecoz2_classify.h")).read()
    for name in ("e2vq_hmm_segment_trans_posteriors(", "e2vq_hmm_segment_trans_posteriors_last_kernel_ms(",
                 "e2vq_hmm_segment_trans_files_posteriors("):
        assert name in header


# ---- compiler metadata (read as test_hmm_posteriors_cpu.py reads its kernels') ------------------------------------------------
VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_posterior_trans.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_posterior_trans.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _meta(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    return lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))


@pytest.mark.parametrize("pattern", [r"k_hmm_loop_posteriors_transILb0ELb0EE", r"k_hmm_loop_posteriors_transILb0ELb1EE",
                                     r"k_hmm_loop_posteriors_transILb1ELb0EE", r"k_hmm_loop_posteriors_transILb1ELb1EE"])
def test_kernels_have_no_scratch_no_spill_and_fit_their_budget(asm, pattern):
    g = _meta(asm, pattern)
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
