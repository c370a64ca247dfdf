"""GPU parity of the HMM kernels at the launch shapes small corpora never reach: the E-step above N = 141 (A read from
global memory), at the LDS limit N = 141, persistent workgroups and waves that loop over several sequences with bad
ones in between, scoring at N = 512, the 2^20-sequence chunks and the split of the models over grid.y, long sequences
and the largest alphabet.  Everything is bit-exact against the oracle (mant / exp2 / status of every sequence, every
accumulator word, every parameter bit, the measure of every iteration); where the issue is the shared algorithm, ln
P(O) and the decoded counts are also compared with the extended-precision restatement (tests/hmm_ld_restatement.py)
within the bounds derived in test_hmm_counts_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import ecoz2rs_amd as e
from tests import hmm_ld_restatement as R
from tests import oracle_lib
from tests.test_hmm_counts_cpu import _without_column, counts_excess, lnp_tolerance

pytestmark = pytest.mark.gpu

FB_WG_GRID = 64  # workgroups of k_hmm_fb_wg: sequence s runs on workgroup s % 64
FB_WAVES = 8192  # waves of k_hmm_fb once S > 8192 (2048 workgroups x 4): sequence s runs on wave s % 8192


@pytest.fixture(scope="module")
def H():
    return oracle_lib.load_hmm()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_estep(H, pi, A, B, seqs):
    """GPU E-step against the oracle, bit for bit: -> (acc, oracle per-sequence results)"""
    acc_o, res = H.accumulate(pi, A, B, seqs)
    acc, mant, ex, st = e.hmm.estep(pi, A, B, seqs)
    assert st.tolist() == [r[0] for r in res]
    assert np.array_equal(_bits(mant), _bits([r[1] for r in res])) and ex.tolist() == [r[2] for r in res]
    assert np.array_equal(acc, acc_o)
    return acc, res


def _bad_mix(rng, M, lens, k_bad, bad_at):
    """random sequences avoiding symbol k_bad (whose column of B the caller zeroes); bad_at: {index: kind} with kind
    'empty' (T = 0), 'range' (a symbol >= M) or 'emit' (k_bad, which no state emits)"""
    good = np.array([k for k in range(M) if k != k_bad])
    seqs = [good[rng.integers(0, len(good), n)].astype(np.uint16) for n in lens]
    for s, kind in bad_at.items():
        x = seqs[s] if len(seqs[s]) >= 2 else good[:3].astype(np.uint16)
        if kind == "empty":
            seqs[s] = np.zeros(0, np.uint16)
        elif kind == "range":
            seqs[s] = np.concatenate([x[:1], [M], x[1:]]).astype(np.uint16)
        else:
            seqs[s] = np.concatenate([x[:1], [k_bad], x[1:]]).astype(np.uint16)
    return seqs


# ---- a. E-step, workgroup kernels ---------------------------------------------------------------------------------
# each workgroup meets good -> bad -> good in its own loop: workgroups 1, 2, 3 at their second sequence, workgroup 10 at
# its first, workgroup 2 again at its third; sequence S - 1 (the last one of its workgroup) is empty
WG_BAD = {FB_WG_GRID + 1: "empty", FB_WG_GRID + 2: "range", FB_WG_GRID + 3: "emit", 10: "emit", 2 * FB_WG_GRID + 2: "empty",
          199: "empty"}


@pytest.mark.parametrize("N,M,typ,hi", [(140, 16, 3, 30), (141, 16, 0, 30), (142, 16, 0, 30), (143, 16, 2, 30),
                                        (200, 16, 1, 20), (511, 8, 3, 9), (512, 8, 0, 9)])
def test_estep_workgroup_kernels(H, N, M, typ, hi):
    """k_hmm_fb_wg<true> up to its LDS limit N = 141, k_hmm_fb_wg<false> from 142 to 512; 200 sequences on 64 persistent
    workgroups, lengths 0, 1, 2 and up, bad sequences between good ones in the same workgroup's loop"""
    H.seed(500 + N)
    rng = np.random.default_rng(N)
    pi, A, B = H.init(N, M, typ)
    B = _without_column(B, M - 1)
    lens = rng.integers(0, hi + 1, 200)
    lens[0], lens[5], lens[7] = 1, 2, 0
    seqs = _bad_mix(rng, M, lens, M - 1, WG_BAD)
    acc, res = _check_estep(H, pi, A, B, seqs)
    assert acc[-1] == sum(r[0] != 0 for r in res) >= len(WG_BAD) + 1 and acc[-2] + acc[-1] == len(seqs)
    assert res[FB_WG_GRID + 1] == (1, 0.5, 1)  # the E-step of an empty sequence: status 1, P = 0.5 * 2^1
    if N in (142, 512):  # the shared algorithm against the independent restatement
        st, lp, cnt, _u, _sk = R.estep(pi, A, B, seqs)
        assert st.tolist() == [r[0] for r in res]
        assert counts_excess(acc, cnt, N, M, seqs, st) <= 1.0
        for s, r in enumerate(res):
            if r[0] == 0:
                assert abs(H.log_prob(r[1], r[2]) - float(lp[s])) <= lnp_tolerance(N, len(seqs[s]), lp[s])


# ---- b. E-step, wave kernel looping over sequences ----------------------------------------------------------------
@pytest.mark.parametrize("N,M,typ,hi", [(5, 32, 0, 40), (64, 16, 3, 10)])
def test_estep_wave_kernel_persistent(H, N, M, typ, hi):
    """k_hmm_fb with S = 20 000 > 8 192 waves: a wave carries its ad / bd / pic registers and used / skipped counts over
    two or three sequences, some of them bad.  (At N = 64 the lengths stop at 10: the oracle's cost, ~3 N^2 per symbol.)"""
    H.seed(600 + N)
    rng = np.random.default_rng(60 + N)
    pi, A, B = H.init(N, M, typ)
    B = _without_column(B, M - 1)
    S = 20_000
    lens = rng.integers(0, hi + 1, S)
    kinds = ("empty", "range", "emit")
    bad = {FB_WAVES + w: kinds[w % 3] for w in range(0, 3000, 7)}  # wave w: good, bad, good
    bad.update({w: kinds[w % 3] for w in range(1, 200, 13)})       # wave w: bad, good, good
    seqs = _bad_mix(rng, M, lens, M - 1, bad)
    acc, res = _check_estep(H, pi, A, B, seqs)
    skipped = sum(r[0] != 0 for r in res)
    assert (acc[-2], acc[-1]) == (S - skipped, skipped) and skipped >= len(bad)


# ---- c. training -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,typ,eps,maxit,S,lo,hi", [(142, 32, 3, 1e-5, 3, 150, 10, 30), (200, 16, 0, 0.0, 2, 100, 5, 20),
                                                       (512, 8, 2, 1e-5, 1, 130, 2, 10)])
def test_training_large_n(H, N, M, typ, eps, maxit, S, lo, hi):
    """E-steps on the workgroup kernel with A in global memory, M-steps, epsilon restriction, stopping rule: the
    parameters and the measure per iteration equal the oracle's bit for bit"""
    H.seed(700 + N)
    rng = np.random.default_rng(70 + N)
    pi, A, B = H.init(N, M, typ)
    seqs = []
    for _ in range(S):
        T = int(rng.integers(lo, hi + 1))
        seqs.append(np.clip((np.linspace(0, M - 1, T) + rng.normal(0, M / 8, T)).round(), 0, M - 1).astype(np.uint16))
    po, Ao, Bo, hist_o = H.learn(pi, A, B, seqs, eps, 0.3, maxit)
    pg, Ag, Bg, hist = e.hmm.train(pi, A, B, seqs, eps, 0.3, maxit)
    assert hist == hist_o and 1 <= len(hist) <= maxit
    for a, b in ((po, pg), (Ao, Ag), (Bo, Bg)):
        assert np.array_equal(_bits(a), _bits(b))
    assert not np.array_equal(_bits(Bo), _bits(B))  # (an M-step ran)


# ---- d. scoring: sizes and splits ----------------------------------------------------------------------------------
def _expect_score(H, models, seqs):
    out = np.zeros((len(seqs), len(models), 3))
    for s, sq in enumerate(seqs):
        for k, m in enumerate(models):
            out[s, k] = H.forward(*m, sq)
    return out


def _assert_score(got, want):
    """got: dict of hmm.score; want (S, K, 3): status, mant, exp2 per pair"""
    assert np.array_equal(got["status"], want[..., 0].astype(np.int32))
    assert np.array_equal(_bits(got["mant"]), _bits(want[..., 1]))
    assert np.array_equal(got["exp2"], want[..., 2].astype(np.int64))


def test_score_n512_with_small_models(H):
    """k_hmm_score_wg with 512 threads, models of N = 512, 1 and 64 in one launch (thread j >= N idle for the small ones)"""
    H.seed(800)
    rng = np.random.default_rng(80)
    M = 8
    models = [H.init(512, M, 0), H.init(1, M, 0), H.init(64, M, 3), H.init(512, M, 2)]
    seqs = [rng.integers(0, M, n).astype(np.uint16) for n in (1, 2, 0, 65, 300, 7, 129)]
    seqs.append(np.array([1, M, 2], np.uint16))
    got = e.hmm.score(models, seqs)
    _assert_score(got, _expect_score(H, models, seqs))
    assert got["status"][7].tolist() == [2] * 4 and got["log_prob"][2].tolist() == [0.0] * 4


def _score_raw(models, sym, offs):
    """e2vq_hmm_score on packed symbols / offsets (hmm.score without the list of arrays)"""
    K, S = len(models), len(offs) - 1
    ms = [tuple(np.ascontiguousarray(x, dtype=np.float64) for x in m) for m in models]
    Ns = (C.c_int * K)(*[len(m[0]) for m in ms])
    ptr = lambda i: (C.c_void_p * K)(*[m[i].ctypes.data for m in ms])
    mant, ex = np.zeros((S, K)), np.zeros((S, K), dtype=np.int64)
    st, lp = np.zeros((S, K), dtype=np.int32), np.zeros((S, K))
    e._lib.check(e.lib.e2vq_hmm_score(0, K, Ns, ms[0][2].shape[1], ptr(0), ptr(1), ptr(2), sym.ctypes.data,
                                      offs.ctypes.data, S, mant.ctypes.data, ex.ctypes.data, st.ctypes.data, lp.ctypes.data))
    return dict(mant=mant, exp2=ex, status=st, log_prob=lp)


def test_score_past_2_pow_20_sequences(H):
    """S = 2^20 + 3 001 sequences on the workgroup path: two launches, the second at s0 = 2^20 (offsets and outputs
    shifted by s0, outputs by s0 * K with K = 2).  The sequences come from a pool of 97 distinct ones (lengths 0 to 3)
    with distinct scores, sequence s = pool[s % 97]: a wrong offset or output index on either side of s0 picks another
    pool entry and shows."""
    H.seed(900)
    rng = np.random.default_rng(90)
    M, P = 16, 97
    models = [H.init(65, M, 0), H.init(3, M, 0)]
    pool = np.zeros((P, 3), dtype=np.uint16)
    plen = np.zeros(P, dtype=np.int64)
    seen = set()
    for p in range(P):
        while True:
            n = [0, 1, 3][p] if p < 3 else int(rng.integers(1, 4))
            row = rng.integers(0, M, 3).astype(np.uint16)
            if p == 2:
                row[1] = M  # one sequence with a symbol outside the alphabet
            key = tuple(row[:n].tolist())
            if key not in seen:
                break
        seen.add(key)
        pool[p], plen[p] = row, n
    want_pool = _expect_score(H, models, [pool[p, :plen[p]] for p in range(P)])
    assert len({tuple(want_pool[p].ravel()) for p in range(P)}) == P  # distinct scores
    S = (1 << 20) + 3001
    idx = np.arange(S) % P
    lens = plen[idx]
    offs = np.zeros(S + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    sym = np.ascontiguousarray(pool[idx][np.arange(3)[None, :] < lens[:, None]])
    assert len(sym) == offs[-1]
    got = _score_raw(models, sym, offs)
    _assert_score(got, want_pool[idx])
    lp_pool = np.array([[H.log_prob(m, int(x)) if st == 0 else -np.inf for st, m, x in row] for row in want_pool])
    assert np.array_equal(got["log_prob"], lp_pool[idx])


@pytest.mark.parametrize("path", ["wave", "workgroup"])
def test_score_more_models_than_grid_y(H, path):
    """K = 65 540 models: grid.y holds 65 535, the last 5 come in a second launch with k0 = 65 535.  The models are
    pool[k % 13] (13 distinct, N from 1 to 13); on the workgroup path model 65 537 is replaced by one with N = 65."""
    H.seed(1000)
    rng = np.random.default_rng(100)
    M, P, K = 4, 13, 65_540
    pool = [H.init(n + 1, M, n % 4 if n % 4 != 1 else 0) for n in range(P)]
    big = H.init(65, M, 0)
    special = 65_537
    models = [pool[k % P] for k in range(K)]
    if path == "workgroup":
        models[special] = big
    seqs = [rng.integers(0, M, 5).astype(np.uint16), np.zeros(0, np.uint16), rng.integers(0, M, 40).astype(np.uint16)]
    got = e.hmm.score(models, seqs)
    want_pool = _expect_score(H, pool, seqs)
    assert len({tuple(want_pool[[0, 2], p].ravel()) for p in range(P)}) == P  # distinct scores
    want = want_pool[:, np.arange(K) % P]
    if path == "workgroup":
        want[:, special] = _expect_score(H, [big], seqs)[:, 0]
    _assert_score(got, want)


# ---- e. long sequences ---------------------------------------------------------------------------------------------
def test_score_long_sequences(H):
    """T = 200 000 at N = 5 (wave path, 3 125 chunks of 64 symbols; and on the workgroup path next to an N = 65 model)
    and at N = 65: bit-exact with the oracle, ln P(O) within the derived bound of the restatement"""
    H.seed(1100)
    rng = np.random.default_rng(110)
    M = 32
    m5, m65 = H.init(5, M, 0), H.init(65, M, 3)
    seq = rng.integers(0, M, 200_000).astype(np.uint16)
    want = _expect_score(H, [m5, m65], [seq])
    _assert_score(e.hmm.score([m5], [seq]), want[:, :1])
    got = e.hmm.score([m5, m65], [seq])
    _assert_score(got, want)
    for k, (m, N) in enumerate(((m5, 5), (m65, 65))):
        st, lp = R.log_prob(*m, seq)
        assert st == 0 and abs(got["log_prob"][0, k] - float(lp)) <= lnp_tolerance(N, len(seq), lp)


@pytest.mark.parametrize("N,M,typ,T", [(5, 32, 0, 50_000), (142, 16, 0, 5_000)])
def test_estep_long_sequence(H, N, M, typ, T):
    """one long sequence next to short ones: bit-exact with the oracle; ln P(O) and the counts within the derived bounds
    of the restatement"""
    H.seed(1200 + N)
    rng = np.random.default_rng(120 + N)
    pi, A, B = H.init(N, M, typ)
    seqs = [rng.integers(0, M, n).astype(np.uint16) for n in (T, 3, 0, 17)]
    acc, res = _check_estep(H, pi, A, B, seqs)
    st, lp, cnt, _u, _sk = R.estep(pi, A, B, seqs)
    assert st.tolist() == [r[0] for r in res] == [0, 0, 1, 0]
    assert abs(H.log_prob(res[0][1], res[0][2]) - float(lp[0])) <= lnp_tolerance(N, T, lp[0])
    assert counts_excess(acc, cnt, N, M, seqs, st) <= 1.0


# ---- f. the largest alphabet -----------------------------------------------------------------------------------------
def test_largest_alphabet(H):
    """M = 65 536 with symbol 65 535 present: the E-step at N = 65 (BN of 65 x 65 536 cells) and scoring at N = 5"""
    H.seed(1300)
    rng = np.random.default_rng(130)
    M = 65_536
    seqs = [rng.integers(0, M, n).astype(np.uint16) for n in (40, 1, 0, 25)]
    seqs[0][[0, 7, 39]] = 65_535
    seqs[1][0] = 65_535
    seqs[3][5] = 0
    pi, A, B = H.init(65, M, 0)
    acc, res = _check_estep(H, pi, A, B, seqs)
    assert [r[0] for r in res] == [0, 0, 1, 0]
    BN = acc[2 * (65 + 65 * 65 + 65):2 * (65 + 65 * 65 + 65 + 65 * M)].reshape(65, M, 2)
    assert np.any(BN[:, 65_535] != 0)
    m5 = H.init(5, M, 3)
    _assert_score(e.hmm.score([m5], seqs), _expect_score(H, [m5], seqs))
