"""`hmm segment --class-transitions --grammar-posteriors` on the GPU where its own file does not take it,
on the inputs of tests/hmm_class_loop_cases.py, the raw bits of post and ln P(O | loop), and status, against the numpy
restatement (no tolerance): a named row for each of the four instantiations of k_hmm_loop_posteriors_trans<A_LDS, W_LDS>,
and for the launch above 64 KB of dynamic LDS in the three that can exceed it -- K up to 1024, 3,776 bytes under the LDS cap,
one-class slots next to packed ones --; with every price -inf the bits of `segment_posteriors` at -inf above 64 KB; a symbol
outside the alphabet and a symbol no state emits at the edges of the 64-symbol hand-out and at the last frame, under one
class set per instantiation, behind a batch of clean streams (every row of a failed stream has to be written) and behind a
chunk that is not the first; the seeded random sets.  Next door, k_hmm_segment_trans<false, true> above 64 KB."""
import numpy as np
import pytest

from ecoz2rs_amd import hmm

from . import hmm_class_loop_cases as cases
from . import hmm_segment_trans_restatement as RT
from . import hmm_trans_posterior_restatement as R
from .test_gpu_hmm_segment_trans import _assert_equal as _assert_trans
from .test_gpu_hmm_trans_posteriors import _assert_equal, _bits

pytestmark = pytest.mark.gpu

NINF = float("-inf")
CHUNK = "ECOZ2_HMM_POSTERIOR_CHUNK_BYTES"


# ---- 1. the rows: every instantiation, and the opt-in above 64 KB in three -------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.TRANS_POSTERIORS_SHAPES))
def test_the_grammar_posteriors_equal_the_restatement_at_every_row(name, monkeypatch):
    monkeypatch.delenv(CHUNK, raising=False)
    models, stream, lt = cases.trans_posteriors_shape(name)
    T, K = len(stream), len(models)
    got = hmm.segment_trans_posteriors(models, stream, [0, T], lt)
    _assert_equal(got, cases.trans_posteriors_reference(name), name)
    assert got["status"].tolist() == [0] and got["post"].shape == (T, K) and T == cases.TRANS_POSTERIORS_T


@pytest.mark.parametrize("name", ["64x3", "64x6_1x84"])  # <true, true> and <false, true>, both above 64 KB
def test_all_prices_minus_infinity_are_the_bits_of_the_single_price_kernel_above_64_kb(name, monkeypatch):
    monkeypatch.delenv(CHUNK, raising=False)
    models, stream, _lt = cases.trans_posteriors_shape(name)
    T, K = len(stream), len(models)
    assert cases.route("trans_posteriors", [len(m[0]) for m in models])["lds"] > cases.LDS_OPT_IN
    got = hmm.segment_trans_posteriors(models, stream, [0, T], np.full((K, K), NINF))
    _assert_equal(got, hmm.segment_posteriors(models, stream, [0, T], NINF), name)
    assert got["status"].tolist() == [0]


# ---- 2. events at the edges of the 64-symbol hand-out ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.TRANS_POSTERIORS_EVENT_SETS)
def test_the_grammar_posteriors_meet_a_bad_and_a_dead_symbol_at_the_edges_of_the_hand_out(name, monkeypatch):
    monkeypatch.delenv(CHUNK, raising=False)
    streams, kinds = cases.event_batch()
    sym, offs = hmm._pack(streams)
    models = cases.event_models(name)
    K, T, S = len(models), cases.EVENT_T, len(streams)
    lt = cases.event_prices(K)
    want = cases.trans_posteriors_event_reference(name)
    # A batch of clean streams goes first: memory the allocator hands out again then holds posteriors, not zeros, and a failed
    # stream's rows are +0.0 only if the kernel writes every one of them (T K entries by a workgroup of 64 threads a slot).
    clean = hmm.segment_trans_posteriors(models, np.tile(sym[:T], S), offs, lt)
    assert clean["status"].tolist() == [0] * S and (clean["post"].sum(axis=1) > 0.99).all()
    got = hmm.segment_trans_posteriors(models, sym, offs, lt)
    _assert_equal(got, want, name)
    # (the first event in frame order decides: (DEAD, M) is 1, (M, DEAD) is 2)
    assert got["status"].tolist() == [0] + [2] * 6 + [1] * 6 + [1, 2] * 3 == [cases.event_status(k, "trans_posteriors") for k in kinds]
    assert np.isfinite(got["log_prob"][0]) and (got["log_prob"][1:] == NINF).all()
    failed = got["post"][T:]
    assert failed.shape == ((S - 1) * T, K) and not failed.any() and not np.signbit(failed).any()
    alone = hmm.segment_trans_posteriors(models, sym[:T], [0, T], lt)
    _assert_equal(alone, dict(post=got["post"][:T], log_prob=got["log_prob"][:1], status=got["status"][:1]), (name, "alone"))
    assert np.array_equal(_bits(clean["post"][:T]), _bits(alone["post"]))
    # The same witness one stream a call: at 350 classes the batch's `post` (6.9 MB) is too large for the allocator to hand
    # the clean batch's memory out again, and a fill that stopped short would meet fresh zeros.  A single stream's 364 KB is
    # handed out again (a scratch build whose fill stops at entry 40,000 fails here, and only here).
    for s in (1, 3, 6, 12, 13, 18):  # M at 0, at 63, at 129; dead at 129; (dead, M) at 0; (M, dead) at 64
        hmm.segment_trans_posteriors(models, sym[:T], [0, T], lt)
        one = hmm.segment_trans_posteriors(models, sym[s * T:(s + 1) * T], [0, T], lt)
        assert one["status"].tolist() == [cases.event_status(kinds[s], "trans_posteriors")] != [0], s
        assert one["post"].shape == (T, K) and not one["post"].any() and not np.signbit(one["post"]).any(), s
    monkeypatch.setenv(CHUNK, "1")  # one stream per launch: a0 of an event stream is not 0
    _assert_equal(hmm.segment_trans_posteriors(models, sym, offs, lt), want, (name, "chunks"))


# ---- 3. the random sets ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_resident():
    return cases.random_sets(cases.RANDOM_SEED, resident_only=True)


# what the draw gives the launcher (asserted, so that a later change of the draw cannot lose it): set -> (A_LDS, W_LDS, bytes or None)
RANDOM_ABOVE_64_KB = {1: (True, True, None), 8: (True, True, None), 11: (True, True, None), 0: (True, False, 161120)}


@pytest.mark.parametrize("i", range(12))  # (a case per set: the restatement of the twelve takes 19 seconds)
def test_the_grammar_posteriors_on_the_random_sets(i, random_resident, monkeypatch):
    monkeypatch.delenv(CHUNK, raising=False)
    row = random_resident[i]
    K = len(row["Ns"])
    if i in RANDOM_ABOVE_64_KB:
        a_lds, w_lds, lds = RANDOM_ABOVE_64_KB[i]
        r = cases.route("trans_posteriors", row["Ns"])
        assert (r["a_lds"], r["w_lds"]) == (a_lds, w_lds) and r["lds"] > cases.LDS_OPT_IN and lds in (None, r["lds"]), r
    sym, offs = hmm._pack(row["streams"])  # the six streams in one call
    lt = cases.forbidding_prices(i, K)
    got = hmm.segment_trans_posteriors(row["models"], sym, offs, lt)
    _assert_equal(got, R.posteriors(row["models"], sym, offs, lt), (i, row["Ns"]))


# ---- 4. the neighbour: k_hmm_segment_trans<A_LDS = false, LT_LDS = true> above 64 KB ---------------------------------------------
def test_segment_trans_with_lA_global_and_lt_in_more_than_64_kb_of_lds(monkeypatch):
    monkeypatch.delenv("ECOZ2_HMM_SEGMENT_CHUNK_BYTES", raising=False)
    models, stream, lt = cases.trans_posteriors_shape("64x6_1x84")
    r = cases.route("trans", [len(m[0]) for m in models])
    assert (r["a_lds"], r["lt_lds"], r["lds"]) == (False, True, 66496) and r["lds"] > cases.LDS_OPT_IN
    T = len(stream)
    got = hmm.segment_trans(models, stream, [0, T], lt)
    _assert_trans(got, RT.segment_trans(models, stream, [0, T], lt), "64x6_1x84")
    assert got["status"].tolist() == [0] and got["entered"].sum() >= 10
