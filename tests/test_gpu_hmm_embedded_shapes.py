"""`hmm learn --embedded` on the GPU where classes and units part: the size of A and of the AN table comes
from the classes; slots, L and sum N come from the transcript.  Every limb of every class's accumulator block, the raw bits of
ln P and the status against the numpy restatement (tests/hmm_embedded_restatement.py), with the comparison of
test_gpu_hmm_embedded.py, at the rows of hmm_align_cases.SHAPES -- the plan's own choice of A and AN in global memory with
one unit and with three units to a wave, units of one state, M = 1024 and M = 65536 --; the order of a symbol outside the
alphabet and a symbol no state emits at the edges of the 64-symbol hand-out (the first event in frame order decides); one
launch of streams that differ in L, sum N and slots; a seeded random batch; and two iterations of the training loop with 48
classes in one M-step launch and at M = 1024."""
import numpy as np
import pytest

from ecoz2rs_amd import hmm

from . import hmm_embedded_cases as cases
from . import hmm_embedded_restatement as R
from .test_gpu_hmm_embedded import _assert_equal, _bits, _both

pytestmark = pytest.mark.gpu

NINF = float("-inf")
ROWS = [name for name in cases.SHAPES if name != "64x6c_17u"]  # (17 slots: the E-step refuses them, test_gpu_hmm_embedded.py)
A_AND_AN_GLOBAL = ("64x6c_8u", "21x48c")


def _opts(opt):
    return None if opt is None else [opt]


# ---- the rows of SHAPES ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS)
def test_the_counts_equal_the_restatement_at_every_shape(name, monkeypatch):
    models, units, opt, stream = cases.shape(name)
    Ns = [len(m[0]) for m in models]
    assert R.slots_of(models, units) == cases.slots_of([Ns[k] for k in units]) <= R.MAX_SLOTS
    both_global = cases.embed_route(Ns, len(units)) == (False, False)
    assert both_global == (name in A_AND_AN_GLOBAL)  # (what embed_plan chooses by itself; every other row: both in LDS)
    assert both_global or cases.embed_route(Ns, len(units)) == (True, True)
    for ls in (0.0, -3.0):
        got, want = _both(models, [stream], [units], _opts(opt), ls=ls)
        _assert_equal(got, want, (name, ls))
        assert got["status"].tolist() == [0] and np.isfinite(got["log_prob"][0])
    forced = []
    if both_global:  # forcing what the plan has already chosen changes nothing
        forced = [("global", "global")]
    if name == "mixed_M1024":
        forced = [(None, "lds"), (None, "global")]
    for a, an in forced:
        if a:
            monkeypatch.setenv("ECOZ2_HMM_EMBED_A", a)
        monkeypatch.setenv("ECOZ2_HMM_EMBED_AN", an)
        _assert_equal(_both(models, [stream], [units], _opts(opt), ls=-3.0)[0], got, (name, a, an))


# ---- the order of the events at the edges of the 64-symbol hand-out ----------------------------------------------------------------
@pytest.mark.parametrize("chunk_bytes", [None, "1"])
def test_the_first_event_in_frame_order_decides_at_the_edges_of_the_hand_out(chunk_bytes, monkeypatch):
    if chunk_bytes:
        monkeypatch.setenv("ECOZ2_HMM_EMBED_CHUNK_BYTES", chunk_bytes)  # a launch per stream
    models = cases.event_models()
    streams, transcripts, optionals, kinds = cases.event_batch()
    assert len(streams) == 19
    got, want = _both(models, streams, transcripts, optionals, ls=-0.5)
    _assert_equal(got, want, chunk_bytes)
    # a symbol >= M: status 2; a symbol no state emits: c_t = 0, status 1; of the two in neighbouring frames the first decides
    assert got["status"].tolist() == [0] + [2] * 6 + [1] * 6 + [1, 2] * 3
    assert [{"clean": 0, "dead": 1, "dead_M": 1}.get(k, 2) for k in kinds] == got["status"].tolist()
    assert np.isfinite(got["log_prob"][0]) and (got["log_prob"][1:] == NINF).all()
    # a status-1 or status-2 stream adds nothing but its mark
    alone, _w = _both(models, streams[:1], transcripts[:1], optionals[:1], ls=-0.5)
    assert np.array_equal(_bits(got["log_prob"][:1]), _bits(alone["log_prob"])) and alone["status"].tolist() == [0]
    for k, (a, b) in enumerate(zip(got["acc"], alone["acc"])):
        assert np.array_equal(a[:-1], b[:-1]) and a[-2] == 1 and (a[-1], b[-1]) == (18, 0), k


# ---- one launch of unlike streams ------------------------------------------------------------------------------------------------
def test_one_launch_of_streams_that_differ_in_L_sumN_and_slots():
    models, streams, transcripts, optionals = cases.unlike_streams()
    assert [R.slots_of(models, u) for u in transcripts] == [1, 2, 8, 3]  # one workgroup shape (8 waves) and one max_L (30) for all
    got, want = _both(models, streams, transcripts, optionals, ls=-1.0)
    _assert_equal(got, want)
    assert got["status"].tolist() == [0, 0, 0, 0]


# ---- a seeded random batch -------------------------------------------------------------------------------------------------------
RANDOM_SEED = 24


def test_a_seeded_random_batch():
    """Seed 24 (the seed of test_gpu_hmm_align_shapes.py; checked on the restatement alone): L is drawn from 1 .. 24 and drawn
    again while the units take more than 16 slots; 40 of 40 streams have status 0, the widest takes 15 slots, 3784 frames in
    all."""
    models, streams, transcripts, optionals = cases.random_batch(RANDOM_SEED, 24, max_slots=R.MAX_SLOTS)
    assert max(R.slots_of(models, u) for u in transcripts) <= R.MAX_SLOTS
    got, want = _both(models, streams, transcripts, optionals, ls=-0.5)
    assert (want["status"] == 0).sum() >= 30
    _assert_equal(got, want, RANDOM_SEED)


# ---- the training loop -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,epsilon", [("21x48c", 1e-5), ("mixed_M1024", 0.0)])
def test_two_iterations_equal_the_restatements_on_the_bits(name, epsilon):
    models, units, opt, stream = cases.shape(name)
    second = cases.shape(name, seed=1)[3]
    assert opt is None and not np.array_equal(stream, second)
    args = cases.pack([stream, second], [units, units])
    got, hist = hmm.train_embedded(models, *args, -1.0, epsilon, -1e300, 2)
    want, whist = R.train(models, *args, -1.0, epsilon, -1e300, 2)
    assert len(hist) == 2 and np.array_equal(_bits(hist), _bits(np.array(whist)))
    for k, (g, w) in enumerate(zip(got, want)):
        for what, a, b in zip(("pi", "A", "B"), g, w):
            assert np.array_equal(_bits(a), _bits(b)), (name, k, what)
    assert hist[1] > hist[0] and not np.array_equal(got[0][2], models[0][2])
