"""HMM E-step and scoring, CPU side: the oracle (oracle/hmm_oracle.c) against an independent extended-precision
restatement (tests/hmm_ld_restatement.py), the restatement against brute-force path enumeration in exact rationals,
and the argument checks of e2vq_hmm_score / e2vq_hmm_estep / e2vq_hmm_train that must refuse bad input before any
device is touched.  The GPU side of the same shapes is in test_gpu_hmm_shapes.py."""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest

import ecoz2rs_amd as e
from tests import hmm_ld_restatement as R
from tests import oracle_lib

U = 2.0 ** -53  # unit roundoff of f64


@pytest.fixture(scope="module")
def H():
    return oracle_lib.load_hmm()


# ---- tolerances ----------------------------------------------------------------------------------------------------
# The oracle's arithmetic, bounded to first order in u = 2^-53 (all terms are non-negative, so no cancellation):
#   forward, per step: N chained fmas, one product with B_j(o_t) and one division by c_t round -- C_t alpha^_t(j), with
#     C_t = c_0 ... c_t the product of the computed scale factors, is alpha_t(j) to within a relative (N + 2) u per step,
#     so within t (N + 2) u after t steps; the computed alpha^_{T-1} sums to 1 within N u, so C_{T-1} = P(O) within
#     (T (N + 2) + N) u.
#   ln P(O) also takes T roundings of the frexp products p * m, and log(mant) + exp2 * M_LN2 adds at most 2 u |ln P|
#     (the product, the representation of ln 2, the final sum):
#         |ln P_oracle - ln P| <= (T (N + 3) + N) u + 3 u |ln P|.
#   backward, per step: two roundings for u_j = (B_j beta^_{t+1}(j)) / c_{t+1} and N chained fmas -- (N + 2) u per step
#     on beta_t(i) / (c_{t+1} ... c_{T-1}).
#   gamma_t(i) = alpha^_t(i) beta^_t(i) = alpha_t(i) beta_t(i) / C_{T-1} with all three errors and one rounding, so
#     within (t (N + 2) + (T - 1 - t) (N + 2) + T (N + 2) + N + 1) u <= (2 T + 1) (N + 4) u; xi_t(i, j) takes two more
#     roundings, which the same bound covers.
#   A count C is a sum of such terms, so it is within (2 T_max + 1) (N + 4) u C of the exact value, plus the limb
#     rounding of fix2 (round to nearest on a 2^-60 grid: at most 2^-61 per term), plus one rounding when the exact limb
#     sum is turned into a double.  n_terms: the used symbols bound the number of terms of every cell.
# The restatement carries 64-bit mantissas (2^11 times finer than u, sums pairwise or over N terms): the factor 1.01
# absorbs its own error and the second-order terms.
def lnp_tolerance(N, T, lnp):
    return 1.01 * (T * (N + 3) + N) * U + 3 * U * abs(float(lnp))


def count_tolerance(N, T_max, n_terms, ref):
    return 1.01 * ((2 * T_max + 1) * (N + 4) + 1) * U * np.abs(ref.astype(np.float64)) + n_terms * 2.0 ** -61


def counts_excess(acc, ref_counts, N, M, seqs, status):
    """max over every cell of |decoded acc - restated count| / tolerance (<= 1: within the bound)"""
    got = R.decode_words(acc, N, M)
    used = [len(s) for s, st in zip(seqs, status) if st == 0]
    T_max, n_terms = max(used, default=0), sum(used)
    worst = 0.0
    for name in ("PI", "AN", "AD", "BN", "BD"):
        ref = ref_counts[name]
        diff = np.abs(got[name].astype(R.LD) - ref).astype(np.float64)
        worst = max(worst, float(np.max(diff / count_tolerance(N, T_max, n_terms, ref))))
    return worst


# ---- restatement vs brute force ------------------------------------------------------------------------------------
def _brute(pi, A, B, seq):
    """every one of the N^T state paths in exact rationals: -> (P(O), PI, AN, AD, BN, BD) as Fractions"""
    N, M = B.shape
    T = len(seq)
    F = lambda x: Fraction(float(x))
    pi, A, B = [F(x) for x in pi], [[F(x) for x in r] for r in A], [[F(x) for x in r] for r in B]
    P = Fraction(0)
    PI, AD, BD = [Fraction(0)] * N, [Fraction(0)] * N, [Fraction(0)] * N
    AN = [[Fraction(0)] * N for _ in range(N)]
    BN = [[Fraction(0)] * M for _ in range(N)]
    for q in itertools.product(range(N), repeat=T):
        w = pi[q[0]] * B[q[0]][seq[0]]
        for t in range(1, T):
            w *= A[q[t - 1]][q[t]] * B[q[t]][seq[t]]
        if w == 0:
            continue
        P += w
        PI[q[0]] += w
        for t in range(T):
            BN[q[t]][seq[t]] += w
            BD[q[t]] += w
            if t < T - 1:
                AD[q[t]] += w
                AN[q[t]][q[t + 1]] += w
    return P, [x / P for x in PI], [[x / P for x in r] for r in AN], [x / P for x in AD], [[x / P for x in r] for r in BN], [x / P for x in BD]


def _exact(x):
    """a long double as the Fraction it is, every one of its 64 mantissa bits"""
    m, ex = np.frexp(R.LD(x))
    return Fraction(int(np.ldexp(m, 64))) * Fraction(2) ** (int(ex) - 64)


@pytest.mark.parametrize("N,M", [(1, 3), (2, 4), (3, 3)])
def test_restatement_equals_brute_force(N, M):
    """the restatement's ln P(O) and expected counts against the sum over all N^T paths, exact: a mistake in the
    restatement itself (an index, a missing term, the scaling) shows here, far above long-double rounding"""
    R.require_extended()
    rng = np.random.default_rng(10 * N + M)
    e.hmm.set_random_seed(50 + N)
    for typ in range(4):
        pi, A, B = e.hmm.init_model(N, M, typ)
        for T in (1, 2, 4, 6):
            seq = rng.integers(0, M, T).astype(np.uint16)
            st, lp, cnt, used, skipped = R.estep(pi, A, B, [seq])
            P, PI, AN, AD, BN, BD = _brute(pi, A, B, [int(x) for x in seq])
            assert st.tolist() == [0] and (used, skipped) == (1, 0)
            # within 2^-56 relative: long double, not double, precision (a few dozen roundings of 2^-64 each)
            assert abs(_exact(np.exp(lp[0])) - P) <= P * 2 ** -56
            for name, exact in (("PI", PI), ("AN", AN), ("AD", AD), ("BN", BN), ("BD", BD)):
                for x, y in zip(np.ravel(cnt[name]), np.ravel(np.array(exact, dtype=object))):
                    assert abs(_exact(x) - y) <= y * 2 ** -56 + Fraction(1, 2 ** 80), (typ, T, name)
    # the restatement's status codes: T = 0, symbol >= M, a step no state can emit (the first failing step decides)
    pi, A, B = e.hmm.init_model(N, M, 0)
    B = B.copy()
    B[:, 0] = 0.0
    seqs = [np.zeros(0, np.uint16), np.array([1, M], np.uint16), np.array([1, 0, M], np.uint16), np.array([M, 0], np.uint16)]
    st, lp, _cnt, used, skipped = R.estep(pi, A, B, seqs)
    assert st.tolist() == [1, 2, 1, 2] and (used, skipped) == (0, 4) and np.all(np.isneginf(lp))
    assert R.log_prob(pi, A, B, seqs[0]) == (0, 0.0)


def test_decoder_is_exact():
    """(hi * 2^31 + lo) * 2^-60 with Python integers: limbs far beyond 53 bits keep every bit until the one rounding"""
    assert R.decode(1 << 29, 0) == 1 and R.decode(0, 1) == Fraction(1, 1 << 60) and R.decode(-1, (1 << 31) - 1) == Fraction(-1, 1 << 60)
    hi, lo = (1 << 40) + 3, -(1 << 33) + 5
    assert R.decode(hi, lo) == Fraction(hi * 2 ** 31 + lo, 2 ** 60)
    acc = np.array([1 << 29, 1, 3 << 28, 0], dtype=np.int64)  # N = M = 1: five cells, then used / skipped
    d = R.decode_words(np.concatenate([acc[:2], acc[:2], acc[:2], acc[2:4], acc[:2], [4, 2]]), 1, 1)
    assert d["PI"][0] == 1 + 2.0 ** -60 and d["BN"][0, 0] == 1.5 and (d["used"], d["skipped"]) == (4, 2)


# ---- oracle vs restatement -----------------------------------------------------------------------------------------
def _corpus(rng, M, lens, k_bad):
    """sequences of the given lengths; symbol k_bad is one no state emits (the caller zeroes its column of B).  Good
    sequences avoid k_bad; the bad ones are: T = 0, a symbol >= M, and k_bad in the middle."""
    good = [k for k in range(M) if k != k_bad]
    seqs = [np.asarray(rng.choice(good, n), dtype=np.uint16) for n in lens]
    seqs[1] = np.zeros(0, np.uint16)
    seqs[len(seqs) // 3] = np.array([good[0], M, good[0]], np.uint16)
    s = seqs[2 * len(seqs) // 3]
    seqs[2 * len(seqs) // 3] = np.concatenate([s[:len(s) // 2], [k_bad], s[len(s) // 2:]]).astype(np.uint16)
    return seqs


def _without_column(B, k):
    B = B.copy()
    B[:, k] = 0.0
    return B / B.sum(1, keepdims=True)


CASES = [  # N, M, model type, sequences, lengths drawn in [lo, hi], plus one sequence of length T_long
    (1, 16, 0, 200, 1, 60, 2000),
    (5, 32, 0, 200, 1, 80, 2000),
    (5, 32, 1, 50, 1, 80, 2000),
    (5, 32, 2, 50, 1, 80, 2000),
    (5, 32, 3, 100, 1, 80, 2000),
    (64, 16, 3, 60, 1, 40, 1000),
    (65, 8, 0, 60, 1, 40, 1000),
    (142, 16, 2, 50, 1, 12, 600),
    (200, 8, 3, 50, 1, 8, 300),
]


@pytest.mark.parametrize("N,M,typ,S,lo,hi,T_long", CASES)
def test_oracle_counts_match_restatement(H, N, M, typ, S, lo, hi, T_long):
    """per sequence the status and ln P(O), and every expected count of the E-step, of the oracle against the
    extended-precision restatement, within the bound derived above -- then the same comparison against a restatement
    of a slightly different corpus (one sequence left out; one symbol changed) must fail it"""
    R.require_extended()
    rng = np.random.default_rng(1000 * N + 10 * M + typ)
    H.seed(400 + N + typ)
    pi, A, B = H.init(N, M, typ)
    k_bad = M - 1
    B = _without_column(B, k_bad)
    lens = [0 if k == 0 else int(x) for k, x in enumerate(rng.integers(lo, hi + 1, S))]
    lens[0], lens[2], lens[3] = 1, 2, T_long  # (lens[1]: the empty sequence)
    seqs = _corpus(rng, M, lens, k_bad)
    acc, res = H.accumulate(pi, A, B, seqs)
    st, lp, cnt, used, skipped = R.estep(pi, A, B, seqs)
    assert [r[0] for r in res] == st.tolist()
    assert (acc[-2], acc[-1]) == (used, skipped) and skipped == 3
    assert res[1] == (1, 0.5, 1)  # T = 0: status 1 with P = 0.5 * 2^1, as the kernels report it
    for s, r in enumerate(res):
        if r[0] == 0:
            assert abs(H.log_prob(r[1], r[2]) - float(lp[s])) <= lnp_tolerance(N, len(seqs[s]), lp[s]), s
    assert counts_excess(acc, cnt, N, M, seqs, st) <= 1.0
    # negative controls: the check is sharp enough to see one sequence, and one symbol
    good = [s for s in range(len(seqs)) if st[s] == 0 and len(seqs[s]) > 1]
    drop = good[len(good) // 2]
    _st, _lp, cnt_drop, _u, _sk = R.estep(pi, A, B, seqs[:drop] + seqs[drop + 1:])
    assert counts_excess(acc, cnt_drop, N, M, seqs, st) > 1.0
    changed = [s.copy() for s in seqs]
    x = changed[drop]
    x[len(x) // 2] = (int(x[len(x) // 2]) + 1) % (M - 1)  # another symbol, still not k_bad = M - 1
    _st, _lp, cnt_sym, _u, _sk = R.estep(pi, A, B, changed)
    assert _st.tolist() == st.tolist()
    assert counts_excess(acc, cnt_sym, N, M, seqs, st) > 1.0


def test_oracle_log_prob_of_a_long_sequence(H):
    """ln P(O) of T = 10^5 symbols at N = 5 (about 3.5 * 10^5 in magnitude) within (T (N + 3) + N) u + 3 u |ln P|"""
    R.require_extended()
    rng = np.random.default_rng(99)
    for typ in (0, 3):
        H.seed(17 + typ)
        pi, A, B = H.init(5, 32, typ)
        seq = rng.integers(0, 32, 100_000).astype(np.uint16)
        st, m, ex = H.forward(pi, A, B, seq)
        rst, rlp = R.log_prob(pi, A, B, seq)
        assert st == rst == 0
        assert abs(H.log_prob(m, ex) - float(rlp)) <= lnp_tolerance(5, len(seq), rlp)
        # sharp: one symbol more shifts ln P by about ln(1 / 32), far above the bound
        assert abs(H.log_prob(m, ex) - float(R.log_prob(pi, A, B, seq[:-1])[1])) > 100 * lnp_tolerance(5, len(seq), rlp)


# ---- argument checks before the device -----------------------------------------------------------------------------
_dp = lambda a: a.ctypes.data_as(C.c_void_p)


def _call(fn, N, M, offs, S):
    pi, A, B = np.full(N, 1.0 / N), np.full((N, N), 1.0 / N), np.full((N, M), 1.0 / M)
    n_sym = max(int(offs.max()), 1)
    sym = np.zeros(n_sym, dtype=np.uint16)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    if fn == "score":
        K = 1
        Ns = (C.c_int * K)(N)
        ptr = lambda a: (C.c_void_p * K)(a.ctypes.data)
        mant, ex = np.zeros(S), np.zeros(S, dtype=np.int64)
        st, lp = np.zeros(S, dtype=np.int32), np.zeros(S)
        rc = e.lib.e2vq_hmm_score(0, K, Ns, M, ptr(pi), ptr(A), ptr(B), _dp(sym), _dp(offs), S, _dp(mant), _dp(ex),
                                  _dp(st), _dp(lp))
    elif fn == "estep":
        acc = np.zeros(max(int(e.lib.e2vq_hmm_acc_words(min(N, 512), min(M, 65536))), 1), dtype=np.int64)
        mant, ex, st = np.zeros(S), np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int32)
        rc = e.lib.e2vq_hmm_estep(0, N, M, _dp(pi), _dp(A), _dp(B), _dp(sym), _dp(offs), S, _dp(acc), _dp(mant), _dp(ex),
                                  _dp(st))
    else:
        hist, n = np.zeros(16), C.c_int()
        rc = e.lib.e2vq_hmm_train(0, N, M, _dp(pi), _dp(A), _dp(B), _dp(sym), _dp(offs), S, 1e-5, 0.3, 2, _dp(hist),
                                  len(hist), C.byref(n))
    e._lib.check(rc)


@pytest.mark.parametrize("fn", ["score", "estep", "train"])
def test_argument_checks_come_before_the_device(fn):
    """offsets that do not start at 0 or that decrease would send the kernels outside their buffers; N and M beyond
    the product's range would overrun its tables: all of it is a plain error, raised before any device is looked for
    (the messages are the argument checks', not "no HIP device")"""
    import ecoz2rs_amd.hmm  # noqa: F401  (declares the argument types)

    with pytest.raises(e.Ecoz2Error, match=r"offs\[0\] = 3, expected 0"):
        _call(fn, 3, 4, np.array([3, 5, 8]), 2)
    with pytest.raises(e.Ecoz2Error, match=r"offs\[2\] = 2 < offs\[1\] = 6"):
        _call(fn, 3, 4, np.array([0, 6, 2, 9]), 3)
    with pytest.raises(e.Ecoz2Error, match="N=513 M=4 out of range"):
        _call(fn, 513, 4, np.array([0, 2]), 1)
    with pytest.raises(e.Ecoz2Error, match="N=2 M=65537 out of range"):
        _call(fn, 2, 65537, np.array([0, 2]), 1)
