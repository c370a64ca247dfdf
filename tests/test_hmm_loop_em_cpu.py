"""`hmm learn --loop`, CPU side: the numpy restatement against the contract transcribed in plain loops,
against an exact Fraction sum of the expected counts over every composite path (the occupancy per state and symbol, the
in-class transitions, the entries through pi, the bigrams), and against the sibling restatements of 4.8.13 for ln P and the
status and of 4.8.14 for the grammar limbs; the identities of the counts; the streams that add nothing; the frozen class and
the class no path reaches; EM on planted data (the sum of ln P never falls, the emissions move towards the planted ones); the
argument checks of the entry points, which run before any HIP call; the CLI's refusals and its usage lines old and new; the
exports; the M-step's results written and read back; the kernel's compiler metadata.  The GPU parity tests are in
test_gpu_hmm_loop_em.py."""
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

from . import hmm_loop_em_restatement as R
from . import hmm_trans_posterior_restatement as R13
from . import hmm_transitions_em_restatement as R14
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


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _marks(accs, models):
    M = np.asarray(models[0][2]).shape[1]
    return [(int(a[R.layout(len(m[0]), M)["used"]]), int(a[R.layout(len(m[0]), M)["skipped"]])) for a, m in zip(accs, models)]


def _counts_only(accs, models):
    M = np.asarray(models[0][2]).shape[1]
    return [a[:R.layout(len(m[0]), M)["used"]] for a, m in zip(accs, models)]


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
            a, b, ta, tb = R.new_accs(models), R.new_accs(models), R14.new_acc(K), R14.new_acc(K)
            got, want = R.estep_one(models, seq, lt, a, ta), R.transcribe(models, seq, lt, b, tb)
            assert got[1] == want[1] == 0 and _bits(got[0]) == _bits(want[0]), (T, mk)
            assert _same(a, b) and np.array_equal(ta, tb), (T, mk)
            assert _marks(a, models) == [(1, 0)] * K and ta[-2:].tolist() == [1, 0]
            if T == 0:
                assert not any(x.any() for x in _counts_only(a, models)) and not ta[:-2].any()
            # without the grammar table: the same state limbs
            c = R.new_accs(models)
            assert R.estep_one(models, seq, lt, c) == got and _same(a, c)
    lt = _matrix("random", K)
    for bad in ([1, M, 2], [M]):
        a, b = R.new_accs(models), R.new_accs(models)
        assert R.estep_one(models, bad, lt, a) == R.transcribe(models, bad, lt, b) == (NINF, 2)
        assert _same(a, b) and not any(x.any() for x in _counts_only(a, models)) and _marks(a, models) == [(0, 1)] * K


def test_a_stream_of_status_1_or_2_adds_only_to_skipped():
    pi, A, B = (x.copy() for x in _uniform(2, 3))
    B[:, 2] = 0.0
    models = [(pi, A, B), (pi[:1] * 2.0, A[:1, :1] * 2.0, B[:1])]
    for one in (R.estep_one, R.transcribe):
        for seq, status in (([0, 2, 1], 1), ([0, 3], 2)):
            accs, acc_t = R.new_accs(models), R14.new_acc(2)
            assert one(models, seq, [[-1.0, -1.0], [-1.0, -1.0]], accs, acc_t) == (NINF, status)
            assert not any(x.any() for x in _counts_only(accs, models)) and _marks(accs, models) == [(0, 1)] * 2
            assert acc_t.tolist() == [0] * 8 + [0, 1]
    r = R.estep(models, [0, 1, 0, 2, 1, 0, 3, 1], [0, 2, 5, 7, 8], np.full((2, 2), -1.0), acc_trans=True)
    assert r["status"].tolist() == [0, 1, 2, 0] and _marks(r["acc"], models) == [(2, 2)] * 2
    clean = R.estep(models, [0, 1, 1], [0, 2, 3], np.full((2, 2), -1.0), acc_trans=True)
    assert _same(_counts_only(r["acc"], models), _counts_only(clean["acc"], models))
    assert np.array_equal(r["acc_trans"][:-2], clean["acc_trans"][:-2])


# ---- ln P, status and the grammar limbs: the bits of the sibling restatements -------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "zeros"])
@pytest.mark.parametrize("Ns", [(1,), (5,) * 13, (21, 22, 64), (3, 5, 4)])
def test_log_prob_status_and_grammar_limbs_are_the_sibling_restatements_bits(kind, Ns):
    M, K = 6, len(Ns)
    models = _models(kind, Ns, M, 23)
    rng = np.random.default_rng(K)
    lens = (0, 1, 2, 65, 130, 3)
    sym = rng.integers(0, M, sum(lens))
    sym[-2] = M  # the last stream: a symbol outside the alphabet
    offs = np.concatenate([[0], np.cumsum(lens)])
    for mk in MATRICES:
        lt = _matrix(mk, K, 1)
        got, want = R.estep(models, sym, offs, lt, acc_trans=True), R13.posteriors(models, sym, offs, lt)
        assert np.array_equal(got["status"], want["status"]) and got["status"].tolist() == [0] * 5 + [2], mk
        assert np.array_equal(_bits(got["log_prob"]), _bits(want["log_prob"])), mk
        assert np.array_equal(got["acc_trans"], R14.estep(models, sym, offs, lt)["acc"]), mk
        assert _marks(got["acc"], models) == [(5, 1)] * K


# ---- brute force: an exact sum of every expected count over every composite path ----------------------------------------------
def _brute(models, seq, lt):
    """exact expected counts (Fractions) and P(O | loop).  One step from (f, i) to (k, j) weighs [f == k] A_f[i][j] +
    w[f][k] pi_k[j]: the first term is the in-class transition i -> j, the second the succession f -> k and the entry of class
    k through pi[j]; a path of weight wt counts wt * (the term) / (the step's weight) for each."""
    F = lambda x: Fraction(float(x))
    K, T = len(models), len(seq)
    M = len(models[0][2][0])
    Ns = [len(m[0]) for m in models]
    w = [[F(math.exp(float(lt[f][k]))) for k in range(K)] for f in range(K)]
    states = [(k, j) for k in range(K) for j in range(Ns[k])]
    gam = [[[Fraction(0)] * M for _ in range(N)] for N in Ns]  # [k][j][o]
    pi0 = [[Fraction(0)] * N for N in Ns]                      # the first entry, [k][j]
    ent = [[Fraction(0)] * N for N in Ns]                      # the entries through pi at t >= 1
    xi = [[[Fraction(0)] * N for _ in range(N)] for N in Ns]   # [k][i][j]
    big = [[Fraction(0)] * K for _ in range(K)]
    total = Fraction(0)
    for path in itertools.product(states, repeat=T):
        k, j = path[0]
        wt = F(models[k][0][j]) * F(models[k][2][j][seq[0]])
        shares = []
        for t in range(1, T):
            k2, j2 = path[t]
            enter = w[k][k2] * F(models[k2][0][j2])
            stay = F(models[k][1][j][j2]) if k2 == k else Fraction(0)
            wt *= (enter + stay) * F(models[k2][2][j2][seq[t]])
            if not wt:
                break
            shares.append((k, j, k2, j2, enter / (enter + stay)))
            k, j = k2, j2
        if not wt:
            continue
        total += wt
        for t, (k, j) in enumerate(path):
            gam[k][j][seq[t]] += wt
        pi0[path[0][0]][path[0][1]] += wt
        for f, i, k2, j2, share in shares:
            big[f][k2] += wt * share
            ent[k2][j2] += wt * share
            if f == k2:
                xi[f][i][j2] += wt * (1 - share)
    div = lambda x: x / total
    deep = lambda t: [deep(x) if isinstance(x, list) else div(x) for x in t]
    return dict(gam=deep(gam), pi0=deep(pi0), ent=deep(ent), xi=deep(xi), big=deep(big)), total


BRUTE_MATRICES = {  # K = 3 (cut to the models' K): asymmetric with -inf entries; a row all -inf; a column all -inf
    "asymmetric": [[-0.5, NINF, -2.0], [-3.0, -0.25, NINF], [NINF, -1.0, -4.0]],
    "row": [[-1.0, -0.5, -2.0], [NINF, NINF, NINF], [-0.25, -3.0, -1.5]],
    "column": [[-1.0, NINF, -2.0], [-0.75, NINF, -0.5], [-0.25, NINF, -1.5]],
    "free": [[0.0] * 3] * 3,
}


def tolerance(T, Nmax, K, terms=None):
    """Derived as 4.8.14 derives its own.  Every count term -- an occupancy ah * bh, an in-class (ah A) u, an entry (m pi) u, a
    bigram S (w R) -- is a product of a forward and a backward quantity of 4.8.13, so that section's first-order bound holds for
    it: every term is non-negative, relative errors add, 2 N + 2 K + 32 bounds a step (the two or three products that form the
    term lie within the 32), 2 T + 1 steps lie between a value and the parameters, the factor 4 covers the second order; a term
    is <= 1, so the relative bound is an absolute one.  A cell sums at most `terms` of them (T for BN, BD and PI, T - 1 for AN
    and the bigrams; T bounds all), each truncated by fix2 to a multiple of 2^-60 (half a unit: 2^-61), and the sum (<= terms)
    is rounded once by unfix."""
    terms = T if terms is None else terms
    per_term = 4.0 * (2 * T + 1) * (2 * Nmax + 2 * K + 32) * U
    return terms * (per_term + 2.0 ** -61) + terms * U


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
            accs, acc_t = R.new_accs(models), R14.new_acc(K)
            lp, st = R.estep_one(models, seq, lt, accs, acc_t)
            R.rowsums(accs, models)
            want, total = _brute(models, seq, lt)
            assert st == 0 and total > 0

            def check(got, exact, what):
                nonlocal worst
                err = abs(float(Fraction(float(got)) - exact))
                worst = max(worst, err / tol)
                assert err <= tol, (T, name, what, err, tol)

            for k, N in enumerate(Ns):
                d = R.decode(accs[k], N, M)
                for j in range(N):
                    for o in range(M):
                        check(d["BN"][j, o], want["gam"][k][j][o], ("BN", k, j, o))
                    check(d["BD"][j], sum(want["gam"][k][j]), ("BD", k, j))
                    check(d["PI"][j], want["pi0"][k][j] + want["ent"][k][j], ("PI", k, j))
                    for i in range(N):
                        check(d["AN"][i, j], want["xi"][k][i][j], ("AN", k, i, j))
                        if models[k][1][i][j] == 0.0:  # an exact zero of A: no limb at all
                            lay = R.layout(N, M)["AN"] + 2 * (i * N + j)
                            assert accs[k][lay] == 0 and accs[k][lay + 1] == 0
                for i in range(N):
                    check(d["AD"][i], sum(want["xi"][k][i]), ("AD", k, i))
                # class k's PI mass over t >= 1 is column k of C
                col = sum(want["big"][f][k] for f in range(K))
                assert sum(want["ent"][k]) == col
                got_col = sum(R14.counts(acc_t, K)[f, k] for f in range(K))
                got_pi = sum(d["PI"]) - float(sum(want["pi0"][k]))
                assert abs(got_pi - got_col) <= (N + K) * tol + 8 * (N + K) * U * T, (T, name, k)
            for f in range(K):
                for k in range(K):
                    check(R14.counts(acc_t, K)[f, k], want["big"][f][k], ("C", f, k))
            lnP = math.log(total.numerator) - math.log(total.denominator)
            assert abs(lp - lnP) <= tol + 4 * U * abs(lnP), (T, name)
    print(f"worst error / tolerance: {worst:.4f}")


# ---- identities ------------------------------------------------------------------------------------------------------------
def test_ad_is_the_integer_row_sum_and_the_occupancy_sums_to_the_frames():
    Ns, M, T = (3, 2, 5, 1), 6, 300
    K = len(Ns)
    models = _models("zeros", Ns, M, 3)
    sym = np.random.default_rng(2).integers(0, M, T)
    r = R.estep(models, sym, [0, T], _matrix("random", K, 4), acc_trans=True)
    assert r["status"].tolist() == [0]
    tol = tolerance(T, max(Ns), K)
    bd_sum, pi_sum = 0.0, 0.0
    for k, N in enumerate(Ns):
        lay, acc = R.layout(N, M), r["acc"][k]
        an = acc[lay["AN"]:lay["AN"] + 2 * N * N].reshape(N, N, 2)
        assert np.array_equal(acc[lay["AD"]:lay["AD"] + 2 * N].reshape(N, 2), an.sum(axis=1))
        d = R.decode(acc, N, M)
        for i in range(N):  # the exact integer, rounded once
            hi, lo = int(an[i, :, 0].sum()), int(an[i, :, 1].sum())
            assert Fraction(float(d["AD"][i])) == Fraction(float(Fraction(hi * (1 << 31) + lo, 1 << 60)))
        assert np.max(np.abs(d["BN"].sum(axis=1) - d["BD"])) <= M * 2.0 ** -60 + 4 * M * U * T  # (BN is truncated cell by cell)
        bd_sum += float(d["BD"].sum())
        pi_sum += float(d["PI"].sum())
    assert abs(bd_sum - T) <= sum(Ns) * tol + 8 * sum(Ns) * U * T, bd_sum
    # every entry through pi is a succession, and frame 0 is one entry more
    c_sum = float(R14.counts(r["acc_trans"], K).sum())
    assert abs(pi_sum - (1.0 + c_sum)) <= (sum(Ns) + K * K) * tol + 8 * (sum(Ns) + K * K) * U * T, (pi_sum, c_sum)


def test_with_every_price_minus_infinity_no_entry_is_counted_after_frame_0():
    Ns, M = (3, 5, 4), 6
    models = _models("random", Ns, M, 2)
    sym = np.random.default_rng(1).integers(0, M, 200)
    r = R.estep(models, sym, [0, 120, 200], np.full((3, 3), NINF), acc_trans=True)
    assert r["status"].tolist() == [0, 0] and not r["acc_trans"][:-2].any()
    pi_sum = sum(float(R.decode(a, N, M)["PI"].sum()) for a, N in zip(r["acc"], Ns))
    assert abs(pi_sum - 2.0) <= 2 * sum(Ns) * tolerance(120, 5, 3, terms=1)  # the first entry of each stream, and nothing else
    free = R.estep(models, sym, [0, 120, 200], np.zeros((3, 3)))
    assert sum(float(R.decode(a, N, M)["PI"].sum()) for a, N in zip(free["acc"], Ns)) > 20.0


# ---- the M-step: frozen and unreached classes --------------------------------------------------------------------------------
def test_a_frozen_class_and_a_class_no_path_reaches_keep_every_byte():
    Ns, M = (3, 2, 3), 6
    models = _models("random", Ns, M, 8)
    # class 2: pi all in a state that cannot emit what the streams hold -- entered, it ends every path
    pi2, A2, B2 = (x.copy() for x in models[2])
    B2[:] = 0.0
    B2[:, 5] = 1.0
    models[2] = (pi2, A2, B2)
    sym = np.random.default_rng(4).integers(0, 5, 160)
    offs = [0, 90, 160]
    r = R.estep(models, sym, offs, _matrix("free", 3))
    assert r["status"].tolist() == [0, 0] and not _counts_only(r["acc"], models)[2].any() and _marks(r["acc"], models)[2] == (2, 0)
    new = R.mstep(models, r["acc"], 0.0, frozen=[1, 0, 0])
    for k in (0, 2):  # the frozen class; the class without a count (epsilon = 0: the floor of B, which `used` > 0 would apply, is off)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(new[k], models[k])), k
    assert not np.array_equal(new[1][2], models[1][2])
    for pi, A, B in new[:2]:
        assert abs(pi.sum() - 1.0) <= 8 * U and np.max(np.abs(A.sum(axis=1) - 1.0)) <= 8 * U
    # the loop: the frozen class stays over the iterations, zeros of pi and A stay zeros
    zs = _models("zeros", Ns, M, 9)
    out, ln_p, hist = R.train(zs, sym, offs, None, ln_switch=-1.0, frozen=[0, 1, 0], epsilon=1e-5, val_auto=1e-9, max_iterations=3)
    assert len(hist) == 3 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(out[1], zs[1])) and not ln_p.any()
    for (pi, A, _B), (zpi, zA, _zB) in zip(out, zs):
        assert not pi[zpi == 0.0].any() and not A[zA == 0.0].any()
    with pytest.raises(ValueError):
        R.train(zs, [6, 6], [0, 2], None)


# ---- EM on planted data ------------------------------------------------------------------------------------------------------
def planted(K=3, N=3, M=16, streams=4, frames=220, seed=7):
    """class models with separated emissions, a grammar that prefers k -> k + 1, and streams drawn from the loop itself: at every
    step the state moves within its class by A or, with the probability that A leaves open, enters a class by the grammar"""
    rng = np.random.default_rng(seed)
    stay = 0.9  # the mass A keeps in the class; the rest switches
    models, true = [], []
    for k in range(K):
        pi = np.array([1.0] + [0.0] * (N - 1))
        A = np.zeros((N, N))
        for i in range(N):
            A[i, i], A[i, min(i + 1, N - 1)] = (0.6, 0.4) if i + 1 < N else (0.0, 1.0)
        B = np.full((N, M), 0.1 / (M - 2))
        for j in range(N):
            B[j, 5 * k + j], B[j, 5 * k + 3] = 0.7, 0.2
        true.append((pi, A, B / B.sum(axis=1, keepdims=True)))
    G = np.full((K, K), 0.1 / (K - 1))
    for k in range(K):
        G[k, (k + 1) % K] = 0.9
    seqs = []
    for _ in range(streams):
        out, k, j = [], int(rng.integers(0, K)), 0
        while len(out) < frames:
            out.append(int(rng.choice(M, p=true[k][2][j])))
            if j == N - 1 and rng.random() > stay:
                k, j = int(rng.choice(K, p=G[k])), 0
            else:
                j = int(rng.choice(N, p=true[k][1][j]))
        seqs.append(np.array(out, dtype=np.uint16))
    for pi, A, B in true:  # the start: the planted rows of B mixed with the uniform row
        models.append((pi.copy(), A.copy(), 0.5 * B + 0.5 / M))
    return true, models, seqs


def _b_distance(models, true):
    return float(sum(np.abs(m[2] - t[2]).sum() for m, t in zip(models, true)))


@pytest.mark.parametrize("train_transitions", [False, True])
def test_em_on_planted_data_never_lowers_the_likelihood(train_transitions):
    true, models, seqs = planted()
    sym, offs = hmm._pack(seqs)
    out, ln_p, hist = R.train(models, sym, offs, None, ln_switch=-2.0, train_transitions=train_transitions, alpha=0.0, epsilon=0.0,
                              val_auto=1e-4, max_iterations=10)
    print("sum ln P per E-step:", ["%.6f" % v for v in hist])
    assert len(hist) >= 3
    for a, b in zip(hist[:-1], hist[1:]):
        assert b - a >= -1e-9 * abs(a), (a, b)  # 4.8.14's margin: the rounding of the sum of ln P, not a licence to fall
    assert hist[-1] > hist[0]
    d0, d1 = _b_distance(models, true), _b_distance(out, true)
    print("summed L1 distance of the B rows to the planted ones: %.4f -> %.4f" % (d0, d1))
    assert d1 < d0  # (a claim the restatement satisfies on this seed; DESIGN.md 4.8.16 holds the figures)
    for pi, A, B in out:
        assert abs(pi.sum() - 1.0) <= 8 * U and np.max(np.abs(A.sum(axis=1) - 1.0)) <= 8 * U and np.max(np.abs(B.sum(axis=1) - 1.0)) <= 32 * U
    if train_transitions:
        assert np.max(np.abs(np.exp(ln_p).sum(axis=1) - 1.0)) <= 16 * U
    else:
        assert not ln_p.any()


# ---- e2vq_hmm_loop_estep / e2vq_hmm_train_loop: refusals before the device -----------------------------------------------------
def _call_c(models, lt, Ns=None, K=None, acc=True, acc_k=True, gram=False, train=False, ln_switch=-1.0, alpha=1.0, epsilon=1e-5):
    Ns = [len(m[0]) for m in models] if Ns is None else Ns
    K = len(models) if K is None else K
    n = max(len(models), 1)
    ns = (C.c_int * n)(*Ns)
    keep = [[np.array(m[i], dtype=np.float64, order="C") for m in models] for i in range(3)]
    ptr = lambda i: (C.c_void_p * n)(*[a.ctypes.data for a in keep[i]])
    sym, offs = np.zeros(8, np.uint16), np.array([0, 8], np.int64)
    lt = None if lt is None else np.ascontiguousarray(lt, dtype=np.float64)
    ltp = lt.ctypes.data if lt is not None else None
    blocks = [np.zeros(R.acc_words(len(m[0]), 8), dtype=np.int64) for m in models]
    accp = (C.c_void_p * n)(*[(b.ctypes.data if acc_k else None) for b in blocks])
    at = np.zeros(2 * n * n + 2, dtype=np.int64)
    if train:
        return e.lib.e2vq_hmm_train_loop(0, K, ns, 8, ptr(0), ptr(1), ptr(2), sym.ctypes.data, offs.ctypes.data, 1, ltp, ln_switch,
                                         int(gram), None, alpha, epsilon, 0.3, 2, None, 0, None,
                                         hmm.HMM_LEARN_CALLBACK(lambda _v, _x: None), 0)
    return e.lib.e2vq_hmm_loop_estep(0, K, ns, 8, ptr(0), ptr(1), ptr(2), sym.ctypes.data, offs.ctypes.data, 1, ltp,
                                     accp if acc else None, at.ctypes.data if gram else None, None, None, 0)


def _bad(where, value):
    pi, A, B = (x.copy() for x in _uniform(3, 8))
    {"pi": pi, "A": A, "B": B}[where].flat[1] = value
    return pi, A, B


W = "e2vq_hmm_loop_estep: "


@pytest.mark.parametrize("case,needle", [
    ("K0", W + "0 models (at least 1)"),
    ("no_lt", W + "bad arguments"),
    ("no_acc", W + "bad arguments"),
    ("no_acc_k", W + "bad arguments"),
    ("N65", W + "model 0 has N=65 states (1 .. 64)"),
    ("lt_nan", W + "lt[1][0] = nan: the logarithm of a price, at most 0 (-inf forbids the succession)"),
    ("lt_pos", W + "lt[0][1] = 0.5: the logarithm of a price, at most 0"),
    ("slots17", W + "the classes take 17 wave-slots of 64 lanes (at most 16: the E-step of the class models under the loop has no looped body)"),
    ("slots17_packed", W + "the classes take 17 wave-slots of 64 lanes (at most 16"),
    ("negative", "HMM parameter A[1] = -0.25: not a finite non-negative number"),
    ("route_an", "ECOZ2_HMM_LOOP_EM_AN=shared: lds or global"),
    ("route_c", "ECOZ2_HMM_LOOP_EM_C=shared: lds or global"),
    ("forced_an", W + "16 classes of 1024 states with the AN table in LDS and the class-to-class table in global memory take"),
    ("forced_c", W + "150 classes of 150 states with the AN table in LDS and the class-to-class table in LDS take"),
])
def test_estep_refuses_before_the_device(case, needle, monkeypatch):
    for k in ("ECOZ2_HMM_LOOP_EM_AN", "ECOZ2_HMM_LOOP_EM_C"):
        monkeypatch.delenv(k, raising=False)
    ok = _uniform(3, 8)
    z = lambda K: np.full((K, K), -1.0)
    if case == "K0":
        rc = _call_c([ok], z(1), K=0)
    elif case == "no_lt":
        rc = _call_c([ok], None)
    elif case == "no_acc":
        rc = _call_c([ok], z(1), acc=False)
    elif case == "no_acc_k":
        rc = _call_c([ok], z(1), acc_k=False)
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
    elif case == "route_an":
        monkeypatch.setenv("ECOZ2_HMM_LOOP_EM_AN", "shared")
        rc = _call_c([ok], z(1))
    elif case == "route_c":
        monkeypatch.setenv("ECOZ2_HMM_LOOP_EM_C", "shared")
        rc = _call_c([ok], z(1))
    elif case == "forced_an":
        monkeypatch.setenv("ECOZ2_HMM_LOOP_EM_AN", "lds")
        rc = _call_c([_uniform(64, 8)] * 16, z(16))
    else:
        monkeypatch.setenv("ECOZ2_HMM_LOOP_EM_C", "lds")
        rc = _call_c([_uniform(1, 8)] * 150, z(150), gram=True)
    assert rc == 1 and needle in _err(), _err()


def test_the_variables_of_the_sibling_trainers_are_not_read(monkeypatch):
    for k in ("ECOZ2_HMM_TRANS_EM_C", "ECOZ2_HMM_EMBED_AN", "ECOZ2_HMM_EMBED_A", "ECOZ2_HMM_EMBED_BODY"):
        monkeypatch.setenv(k, "shared")
    rc = _call_c([_uniform(64, 8)] * 17, np.full((17, 17), -1.0))
    assert rc == 1 and "17 wave-slots" in _err(), _err()  # (the plan ran past the routes to the slot count's refusal ... )
    rc = _call_c([_uniform(3, 8)], [[-1.0]], gram=True)
    assert "shared" not in _err()  # ( ... and a call that passes every host check names none of them)


def test_train_refuses_before_the_device():
    ok, z = _uniform(3, 8), np.full((2, 2), -1.0)
    who = "e2vq_hmm_train_loop: "
    assert _call_c([ok, ok], z, train=True, ln_switch=0.5) == 1 and who + "ln_switch = 0.5" in _err(), _err()
    assert _call_c([ok, ok], z, train=True, alpha=-1.0) == 1 and who + "alpha = -1: a finite number, at least 0" in _err(), _err()
    assert _call_c([ok, ok], z, train=True, epsilon=-1.0) == 1 and who + "epsilon = -1: a finite number, at least 0" in _err(), _err()
    assert _call_c([ok, ok], z, train=True, epsilon=float("nan")) == 1 and who + "epsilon = nan" in _err(), _err()
    assert _call_c([_uniform(64, 8)] * 17, np.full((17, 17), -1.0), train=True) == 1 and who + "the classes take 17 wave-slots" in _err()
    assert _call_c([ok, ok], None, train=True) == 1 and who + "bad arguments" in _err()


def test_sixteen_slots_are_accepted_as_far_as_the_device():
    rc = _call_c([_uniform(64, 8)] * 16, np.full((16, 16), -1.0), gram=True)
    if e.lib.e2vq_device_count() > 0:
        assert rc == 0, _err()
    else:
        assert rc == 1 and "no HIP device" in _err(), _err()


def test_python_mirror_raises_the_refusal():
    sym = np.zeros(8, np.uint16)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.loop_estep([_uniform(3, 8)], sym, [0, 8], [[1.0]])
    assert "lt[0][0] = 1" in str(ei.value)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.train_loop([_uniform(64, 8)] * 17, sym, [0, 8])
    assert "17 wave-slots" in str(ei.value)
    with pytest.raises(ValueError):
        hmm.loop_estep([_uniform(3, 8)] * 2, sym, [0, 8], np.zeros((3, 3)))
    with pytest.raises(ValueError):
        hmm.loop_estep([_uniform(3, 8)] * 2, sym, [0, 8], np.zeros((2, 2)), acc_trans=np.zeros(9, dtype=np.int64))
    with pytest.raises(ValueError):
        hmm.train_loop([_uniform(3, 8)] * 2, sym, [0, 8], frozen=[1, 0, 0])


# ---- the file form and the CLI ----------------------------------------------------------------------------------------------
@pytest.fixture
def corpus(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    models = []
    for c, N in (("A", 3), ("B", 5)):
        hmm.save_model(d / f"{c}.hmm", c, *_uniform(N, 16))
        models.append(str(d / f"{c}.hmm"))
    hmm.save_model(d / "A2.hmm", "A", *_uniform(2, 16))
    (d / "many").mkdir()
    for k in range(17):
        hmm.save_model(d / "many" / f"c{k:02d}.hmm", f"c{k:02d}", *_uniform(64, 16))
    e.formats.write_seq(str(d / "x.seq"), "A", 16, np.arange(40) % 16)
    (d / "t.csv").write_text("class,A,B\nA,0,-1\nB,-2,-inf\n")
    (d / "tpos.csv").write_text("class,A,B\nA,0,-1\nB,2,-inf\n")
    return tmp_path, d, models


def test_files_refuse_before_the_device(corpus):
    tmp_path, d, models = corpus
    who = "e2vq_hmm_learn_loop_files: "
    out, x = tmp_path / "out", [str(d / "x.seq")]
    many = [str(d / "many" / f"c{k:02d}.hmm") for k in range(17)]

    def call(models, inputs, ls=-5.0, out=out, **kw):
        try:
            hmm.learn_loop_files(models, inputs, out if out else "", ls, max_iterations=2, **kw)
        except e.Ecoz2Error as ex:
            return str(ex)
        return ""

    assert who + "the classes take 17 wave-slots of 64 lanes (at most 16: the E-step of the class models under the loop" in call(many, x)
    assert who + "no models" in call([], x)
    assert who + "no inputs" in call(models, [])
    assert who + "no output directory" in call(models, x, out=None)
    assert who + "ln_switch = 2" in call(models, x, ls=2.0)
    assert who + "alpha = -0.5" in call(models, x, alpha=-0.5, train_transitions=True)
    assert who + "epsilon = -1" in call(models, x, hmm_epsilon=-1.0)
    assert "tpos.csv:3: B -> A = 2" in call(models, x, class_transitions=d / "tpos.csv")
    assert "nowhere.csv" in call(models, x, class_transitions=d / "nowhere.csv")
    assert who + "--freeze C: no model has this class" in call(models, x, freeze=["A", "C"])
    assert who + "two models of the class 'A'" in call(models + [str(d / "A2.hmm")], x)
    assert who + str(d / "A.hmm") + " would overwrite an input model" in call(models, x, out=d)
    assert not out.exists()


def _cli(cwd, *args):
    r = subprocess.run([EXE, "hmm", "learn", *args], cwd=cwd, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


MODELS = ["-m", "in/A.hmm", "in/B.hmm"]
TAIL = ["-o", "out", "--sequences", "in/x.seq"]


@pytest.mark.parametrize("args,code,needle", [
    (["--loop"] + MODELS + TAIL, 2, "hmm learn --loop: --switch-penalty <x <= 0 | -inf> is required"),
    (["--loop"] + MODELS + ["--switch-penalty", "1"] + TAIL, 2, "--switch-penalty 1: at most 0"),
    (["--loop"] + MODELS + ["--switch-penalty", "-1", "--sequences", "in/x.seq"], 2, "hmm learn --loop: -o <dir> is required"),
    (["--loop"] + MODELS + ["--switch-penalty", "-1", "-o", "out", "--predictors", "in/x.prd"], 2, "need --codebook <cbook>"),
    (["--loop"] + MODELS + ["--switch-penalty", "-1", "--alpha", "2"] + TAIL, 2, "hmm learn --loop: --alpha needs --train-transitions"),
    (["--loop"] + MODELS + ["--switch-penalty", "-1", "--train-transitions", "--alpha", "-1"] + TAIL, 2, "--alpha -1: at least 0"),
    (["--loop"] + MODELS + ["--switch-penalty", "-1"], 2, "exactly one of --signals, --predictors and --sequences is required"),
    (["--loop", "--embedded"] + MODELS + ["--switch-penalty", "-1"] + TAIL, 2, "hmm learn --loop excludes --embedded"),
    (["--loop", "--labels", "l.csv"] + MODELS + ["--switch-penalty", "-1"] + TAIL, 2, "hmm learn --loop excludes --labels"),
    (["--loop", "--filler", "A"] + MODELS + ["--switch-penalty", "-1"] + TAIL, 2, "hmm learn --loop excludes --filler"),
    (["--loop", "--all-classes"] + MODELS + ["--switch-penalty", "-1"] + TAIL, 2, "hmm learn --loop excludes --all-classes"),
    (["--loop", "--grid"] + MODELS + ["--switch-penalty", "-1"] + TAIL, 2, "hmm learn --loop excludes --grid"),
    (["--loop", "--class-name", "A"] + MODELS + ["--switch-penalty", "-1"] + TAIL, 2, "hmm learn --loop excludes --class-name"),
    (["-M", "16", "--train-transitions", "in/x.seq"], 2, "hmm learn: --train-transitions needs --loop"),
    (["-M", "16", "--freeze", "A", "in/x.seq"], 2, "hmm learn: --freeze needs --loop"),
    (["--embedded", "--freeze", "A"] + MODELS + ["--labels", "l.csv"] + TAIL, 2, "hmm learn: --freeze needs --loop"),
    # past the flags: the library's refusals, exit status 1 on stdout
    (["--loop"] + MODELS + ["--switch-penalty", "-1", "--class-transitions", "in/tpos.csv"] + TAIL, 1, "in/tpos.csv:3: B -> A = 2"),
    (["--loop"] + MODELS + ["--switch-penalty", "-1", "--freeze", "C"] + TAIL, 1, "--freeze C: no model has this class"),
    (["--loop"] + MODELS + ["in/A2.hmm", "--switch-penalty", "-1"] + TAIL, 1, "two models of the class 'A'"),
    (["--loop"] + MODELS + ["--switch-penalty", "-1", "-o", "in", "--sequences", "in/x.seq"], 1, "would overwrite an input model"),
    (["--loop", "-m", "in/many", "--switch-penalty", "-inf"] + TAIL, 1, "the classes take 17 wave-slots of 64 lanes"),
])
def test_cli_refusals(corpus, args, code, needle):
    tmp_path, _d, _models = corpus
    rc, out, err = _cli(tmp_path, *args)
    assert rc == code and needle in (err if code == 2 else out), (rc, out, err)
    assert not (tmp_path / "out").exists()


def test_usage_has_the_lines_old_and_new(tmp_path):
    rc, _out, err = _cli(tmp_path, "--loop")
    assert rc == 2
    old = ("  ecoz2 hmm learn --embedded -m|--models <files|dirs>... --labels <files>... [--filler <class>] [--switch-penalty <x <= 0>]\n"
           "                  [-e 1e-05] [-a 0.3] [-I -1] -o <dir> [--codebook <cbook>] [-P 36] [-W 45] [-O 15]\n"
           "                  [--body <auto|resident|looped>]\n"
           "                  (--signals <.wav files>... | --predictors <.prd files>... | --sequences <.seq files>...)\n"
           "                  (the given models re-estimated from whole recordings and the order of their units, no boundaries:\n"
           "                  label file i is recording i's transcript, as `hmm align` reads it; the models go to <dir>/<class>.hmm)\n")
    new = ("  ecoz2 hmm learn --loop -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15] --switch-penalty <x <= 0 | -inf>\n"
           "                  [--class-transitions <file.csv>] [--train-transitions [--alpha 1]] [--freeze <class>]... [-e 1e-05] [-a 0.3]\n"
           "                  [-I -1] -o <dir> --sequences <.seq>... | --predictors <.prd>... | --signals <.wav>...\n")
    after = "  ecoz2 hmm classify [-r] [-c|--c12n <out.csv>] -m|--models <files|dirs>... --tt <TRAIN|TEST> -M <M> [--class-name c]\n"
    assert old + new in err and after in err and err.index(new) < err.index(after)
    first = ("  ecoz2 hmm learn [-N 5] -M <M> [-t 3] [-I -1] [-e 1e-05] [-a 0.3] [-s <seed>] [--ser] [--class-name c]\n"
             "                  --sequences <file.seq|dirs|tt.csv>...\n"
             "  ecoz2 hmm learn --all-classes [-N 5] -M <M> [-t 3] [-I -1] [-e 1e-05] [-a 0.3] [-s <seed>]\n")
    assert first in err


def test_library_exports():
    names = ("e2vq_hmm_loop_estep", "e2vq_hmm_loop_estep_last_kernel_ms", "e2vq_hmm_train_loop", "e2vq_hmm_learn_loop_files")
    header = open(os.path.join(ROOT, "include", "ecoz2_classify.h")).read()
    for name in names:
        assert hasattr(e.lib, name) and "int " + name + "(" in header
    for fn in ("loop_estep", "loop_estep_last_kernel_ms", "train_loop", "learn_loop_files"):
        assert callable(getattr(hmm, fn))
    ms = C.c_float(0.0)
    assert e.lib.e2vq_hmm_loop_estep_last_kernel_ms(None) == 1 and "bad arguments" in _err()
    assert e.lib.e2vq_hmm_loop_estep_last_kernel_ms(C.byref(ms)) == 0


def test_the_m_steps_results_round_trip_through_their_files(tmp_path):
    K, Ns, M = 3, (2, 3, 2), 6
    models = _models("zeros", Ns, M, 9)
    sym = np.random.default_rng(5).integers(0, M, 150)
    start = np.log(np.full((K, K), 1.0 / K))
    start[1, 2] = NINF
    out, ln_p, hist = R.train(models, sym, [0, 150], start, ln_switch=-1.0, train_transitions=True, alpha=0.25, val_auto=1e-9, max_iterations=2)
    assert len(hist) == 2
    names = ["rain", "ship", "whale"]
    hmm.write_class_transitions(tmp_path / "transitions.csv", names, ln_p)
    back = hmm.read_class_transitions(tmp_path / "transitions.csv", names)
    assert np.array_equal(_bits(back), _bits(ln_p)) and back[1, 2] == NINF and (back <= 0.0).all()
    for c, m in zip(names, out):
        hmm.save_model(tmp_path / f"{c}.hmm", c, *m)
        cls, pi, A, B = hmm.load_model(tmp_path / f"{c}.hmm")
        assert cls == c and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((pi, A, B), m))


# ---- compiler metadata (read as test_hmm_transitions_em_cpu.py reads its kernel's) ---------------------------------------------
VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_loop_estep.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_loop_estep.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _meta(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    return lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))


@pytest.mark.parametrize("pattern", [r"k_hmm_loop_estepILb%dELb%dELb%dEE" % bits for bits in itertools.product((0, 1), repeat=3)])
def test_kernels_have_no_scratch_no_spill_and_fit_their_budget(asm, pattern):
    g = _meta(asm, pattern)
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
    print(pattern, "vgpr", g("vgpr_count"), "sgpr", g("sgpr_count"))
