"""`hmm align` on the GPU where classes and units part: the size of lA, and so whether it lives in LDS,
comes from the classes; slots, L and sum N come from the transcript.  Every output against the numpy restatement
(tests/hmm_align_restatement.py) on the bits, with the comparison of test_gpu_hmm_align.py, at the rows of
hmm_align_cases.SHAPES -- lA in global memory under the resident body with one unit and with three units to a wave
(k_hmm_align<false,false>) and under the looped body (<true,false>), units of one state (64 to a slot, L in the hundreds, a
partly filled last slot, one-state slots next to a 64-state unit), M = 1024 and M = 65536 --; a symbol outside the alphabet and
a symbol no state emits at the edges of the 64-symbol hand-out; one resident launch of streams that differ in L, sum N and
slots; a seeded random batch that interleaves looped launches with resident ones."""
import numpy as np
import pytest

from . import hmm_align_cases as cases
from .test_gpu_hmm_align import _assert_equal, _bits, _both

pytestmark = pytest.mark.gpu

NINF = float("-inf")


# ---- the rows of SHAPES ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.SHAPES))
def test_align_equals_the_restatement_at_every_shape(name):
    models, units, opt, stream = cases.shape(name)
    for ls in (0.0, -3.0):
        got, want = _both(models, [stream], [units], None if opt is None else [opt], ls=ls)
        _assert_equal(got, want, (name, ls))
        assert got["status"].tolist() == [0] and np.isfinite(got["log_prob"][0])
        if opt is None:
            assert (got["begin"] >= 0).all()
        else:  # (T < L: the path has to pass over optional units, and never over a mandatory one)
            assert len(stream) < len(units) and (got["begin"] >= 0)[opt == 0].all() and not (got["begin"] >= 0).all()
    if name == "small_M65536":  # the top symbol is a legal one, on both sides of a hand-out
        assert stream[10] == stream[64] == 65535


@pytest.mark.parametrize("name", ["64x6c_8u", "21x48c"])
def test_the_looped_body_reads_lA_from_global_memory_as_the_resident_body_does(name, monkeypatch):
    models, units, opt, stream = cases.shape(name)
    assert cases.A_GLOBAL[name] == "resident"
    one, want = _both(models, [stream], [units], ls=-1.0)
    _assert_equal(one, want, name)
    monkeypatch.setenv("ECOZ2_HMM_ALIGN_BODY", "looped")  # (lA stays in global memory: d of two steps comes on top)
    _assert_equal(_both(models, [stream], [units], ls=-1.0)[0], one, (name, "looped"))


# ---- events at the edges of the 64-symbol hand-out -------------------------------------------------------------------------------
@pytest.mark.parametrize("body", ["resident", "looped"])
def test_a_bad_symbol_and_a_dead_symbol_at_the_edges_of_the_hand_out(body, monkeypatch):
    monkeypatch.setenv("ECOZ2_HMM_ALIGN_BODY", body)
    models = cases.event_models()
    streams, transcripts, optionals, kinds = cases.event_batch()
    assert len(streams) == 19
    alone, _w = _both(models, streams[:1], transcripts[:1], optionals[:1], ls=-0.5)
    got, want = _both(models, streams, transcripts, optionals, ls=-0.5)
    _assert_equal(got, want, body)
    # any symbol >= M is status 2 wherever it stands; a symbol no state emits leaves no path: status 1
    assert got["status"].tolist() == [0] + [2] * 6 + [1] * 6 + [2, 2] * 3
    assert [{"clean": 0, "dead": 1}.get(k, 2) for k in kinds] == got["status"].tolist()
    assert np.isfinite(got["log_prob"][0]) and (got["log_prob"][1:] == NINF).all()
    T, L = cases.EVENT_T, len(transcripts[0])
    for key in ("unit", "state", "entered", "score"):
        assert np.array_equal(_bits(got[key][:T]), _bits(alone[key]))
    for key in ("begin", "end"):
        assert np.array_equal(got[key][:L], alone[key])
    assert np.array_equal(_bits(got["log_prob"][:1]), _bits(alone["log_prob"])) and alone["status"].tolist() == [0]


# ---- a resident launch of unlike streams -----------------------------------------------------------------------------------------
def test_one_resident_launch_of_streams_that_differ_in_L_sumN_and_slots():
    models, streams, transcripts, optionals = cases.unlike_streams()
    Ns = [len(m[0]) for m in models]
    slots = [cases.slots_of([Ns[k] for k in u]) for u in transcripts]
    # Every stream takes at most 16 slots, so all are resident; align_plan puts consecutive streams of one body into one
    # launch while their tables fit the budget (a few hundred KB here, of 4 GiB) and their largest L and sum N fit LDS: one
    # launch of 8 waves with max_L = 30 and max_sumN = 512, in which three streams have fewer slots than the workgroup has
    # waves and every stream but one an L below max_L.
    assert slots == [1, 2, 8, 3] and [len(u) for u in transcripts] == [1, 13, 8, 30] and [len(s) for s in streams] == [5, 64, 129, 65]
    assert cases.align_route(Ns, transcripts[2]) == (False, True)  # (three classes of 64: lA still fits LDS)
    got, want = _both(models, streams, transcripts, optionals, ls=-1.0)
    _assert_equal(got, want)
    assert got["status"].tolist() == [0, 0, 0, 0]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])])
    uoffs = np.concatenate([[0], np.cumsum([len(u) for u in transcripts])])
    for s in range(4):
        alone, _w = _both(models, streams[s:s + 1], transcripts[s:s + 1], optionals[s:s + 1], ls=-1.0)
        for key in ("unit", "state", "entered", "score"):
            assert np.array_equal(_bits(got[key][offs[s]:offs[s + 1]]), _bits(alone[key])), (s, key)
        for key in ("begin", "end"):
            assert np.array_equal(got[key][uoffs[s]:uoffs[s + 1]], alone[key]), (s, key)
        assert np.array_equal(_bits(got["log_prob"][s:s + 1]), _bits(alone["log_prob"]))


# ---- a seeded random batch -------------------------------------------------------------------------------------------------------
RANDOM_SEED = 24


def test_a_seeded_random_batch_interleaves_looped_and_resident_launches():
    """Seed 24 (the first of 0, 1, 2, .. whose draw has five streams of more than 16 slots; chosen on the restatement alone):
    40 of 40 streams have status 0, 5 take more than 16 slots (at most 20), 33 take fewer than 16, no stream is shorter than
    its transcript, 3320 frames in all."""
    models, streams, transcripts, optionals = cases.random_batch(RANDOM_SEED, 40)
    slots = np.array([cases.slots_of([cases.RANDOM_NS[k] for k in u]) for u in transcripts])
    got, want = _both(models, streams, transcripts, optionals, ls=-0.5)
    assert (want["status"] == 0).sum() >= 30 and (slots > 16).sum() >= 5 and (slots < 16).sum() >= 5
    looped = slots > 16
    assert (looped[1:] != looped[:-1]).sum() >= 4  # (the bodies alternate: a launch ends wherever they change)
    _assert_equal(got, want, RANDOM_SEED)
