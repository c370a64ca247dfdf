"""The looped body of the embedded E-step on the GPU (ECOZ2_HMM_EMBED_BODY): every limb of every class's
accumulator block, the raw bits of ln P and the status against the numpy restatement (tests/hmm_embedded_restatement.py, its
slot bound lifted), no tolerance -- above 16 slots (a wave with two and with three slots, A in global memory); the looped
body forced below 17 slots, where it must also equal the resident body's words; both instantiations and both AN routes
forced; the lengths around the 64-symbol hand-out and T = L; the order of the events; batches under `auto`, whose launches
are cut where the body changes; the training loop and the file form under `auto`; and the default, which still refuses."""
import functools

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_embedded_cases as cases
from . import hmm_embedded_looped_cases as LC
from . import hmm_embedded_restatement as R
from .test_gpu_hmm_embedded import _assert_equal, _bits

pytestmark = pytest.mark.gpu

NINF = float("-inf")
M = cases.M


@pytest.fixture(autouse=True)
def _setup(monkeypatch):
    for k in (LC.BODY, "ECOZ2_HMM_EMBED_A", "ECOZ2_HMM_EMBED_AN", "ECOZ2_HMM_EMBED_CHUNK_BYTES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(R, "MAX_SLOTS", 64)  # (the restatement's arithmetic covers any slot count)


def _run(body, models, streams, transcripts, optionals=None, ls=0.0):
    return hmm.embedded_estep(models, *cases.pack(streams, transcripts, optionals), ls, body=body)


def _want(models, streams, transcripts, optionals=None, ls=0.0):
    return R.estep(models, *cases.pack(streams, transcripts, optionals), ls)


def _opts(opt):
    return None if opt is None else [opt]


def _case(name):
    """-> (models, units, optional or None, stream) of a packing, a shape or the 33-slot case"""
    if name == "33 slots":
        models, units, stream = LC.thirty_three_slots()
        return models, units, None, stream
    if name in cases.PACKINGS:
        models, units, stream = cases.packing(name)
        return models, units, None, stream
    return cases.shape(name)


# ---- above 16 slots ----------------------------------------------------------------------------------------------------------------
ABOVE = {"64x17": (17, (True, False)), "33x20": (20, (True, True)), "64x6c_17u": (17, (False, False)), "33 slots": (33, (True, False))}


@pytest.mark.parametrize("name", list(ABOVE))
def test_the_counts_equal_the_restatement_above_sixteen_slots(name):
    models, units, opt, stream = _case(name)
    Ns = [len(m[0]) for m in models]
    slots, route = ABOVE[name]
    assert R.slots_of(models, units) == slots
    assert LC.looped_route(Ns, len(units), slots, sum(Ns[k] for k in units)) == route  # (A_LDS, the AN table in LDS)
    for ls in (0.0, -3.0):
        got, want = _run("auto", models, [stream], [units], _opts(opt), ls), _want(models, [stream], [units], _opts(opt), ls)
        _assert_equal(got, want, (name, ls))
        assert got["status"].tolist() == [0] and np.isfinite(got["log_prob"][0])
    _assert_equal(_run("looped", models, [stream], [units], _opts(opt), -3.0), got, (name, "looped"))
    assert hmm.embedded_last_kernel_ms() > 0.0


# ---- the looped body forced below 17 slots: the resident body's words ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["5x13", "mixed", "1x3c_200u", "1x3c_201u_opt", "1_64_1", "mixed_M1024"])
def test_the_forced_looped_body_gives_the_resident_bodys_words(name, monkeypatch):
    models, units, opt, stream = _case(name)
    assert R.slots_of(models, units) <= 16
    want = _want(models, [stream], [units], _opts(opt), -1.0)
    resident = _run("resident", models, [stream], [units], _opts(opt), -1.0)
    looped = _run("looped", models, [stream], [units], _opts(opt), -1.0)
    _assert_equal(looped, want, name)
    _assert_equal(looped, resident, (name, "resident"))
    assert want["status"].tolist() == [0]
    if name == "mixed_M1024":
        for an in ("lds", "global"):
            monkeypatch.setenv("ECOZ2_HMM_EMBED_AN", an)
            _assert_equal(_run("looped", models, [stream], [units], _opts(opt), -1.0), want, (name, an))


# ---- forced routes -----------------------------------------------------------------------------------------------------------------
def test_both_instantiations_and_both_an_routes_forced(monkeypatch):
    models, units, _opt, stream = _case("33x20")
    want = _want(models, [stream], [units], None, -1.0)
    for a in ("lds", "global"):
        for an in ("lds", "global"):
            monkeypatch.setenv("ECOZ2_HMM_EMBED_A", a)
            monkeypatch.setenv("ECOZ2_HMM_EMBED_AN", an)
            _assert_equal(_run("auto", models, [stream], [units], None, -1.0), want, (a, an))
    # a forced layout that does not fit is refused: the AN table of three 64-state classes next to 17 x 64 states
    models, units, _opt, stream = _case("64x17")
    monkeypatch.delenv("ECOZ2_HMM_EMBED_A")
    monkeypatch.setenv("ECOZ2_HMM_EMBED_AN", "lds")
    with pytest.raises(Exception, match=r"17 units of sum N = 1088 states in 17 wave-slots, A in global memory and the AN table in LDS take "
                                        r"\d+ bytes of LDS \(at most 163840\)"):
        _run("auto", models, [stream], [units])


# ---- the hand-out's edges and T = L ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 10, 63, 64, 65, 129])
def test_lengths_around_the_hand_out_and_at_the_mandatory_units(T):
    """T = 10 with every other unit optional: as many frames as mandatory units.  T = 1 has no path: status 1."""
    models, units, _opt, stream = _case("33x20")
    opt = np.array([l % 2 for l in range(20)], np.uint8) if T == 10 else None
    got, want = _run("auto", models, [stream[:T]], [units], _opts(opt), -0.5), _want(models, [stream[:T]], [units], _opts(opt), -0.5)
    _assert_equal(got, want, T)
    assert got["status"].tolist() == [1 if T == 1 else 0]


@functools.lru_cache(maxsize=None)
def _events():
    models = cases.event_models()
    streams, transcripts, optionals, kinds = cases.event_batch()
    return models, streams, transcripts, optionals, kinds, _want(models, streams, transcripts, optionals, -0.5)


@pytest.mark.parametrize("chunk_bytes", [None, "1"])
def test_the_first_event_in_frame_order_decides_in_the_looped_body(chunk_bytes, monkeypatch):
    if chunk_bytes:
        monkeypatch.setenv("ECOZ2_HMM_EMBED_CHUNK_BYTES", chunk_bytes)  # a launch per stream
    models, streams, transcripts, optionals, kinds, want = _events()
    assert len(streams) == 19
    got = _run("looped", models, streams, transcripts, optionals, -0.5)
    _assert_equal(got, want, chunk_bytes)
    assert got["status"].tolist() == [0] + [2] * 6 + [1] * 6 + [1, 2] * 3
    assert [{"clean": 0, "dead": 1, "dead_M": 1}.get(k, 2) for k in kinds] == got["status"].tolist()
    assert np.isfinite(got["log_prob"][0]) and (got["log_prob"][1:] == NINF).all()
    alone = _run("looped", models, streams[:1], transcripts[:1], optionals[:1], -0.5)
    assert np.array_equal(_bits(got["log_prob"][:1]), _bits(alone["log_prob"])) and alone["status"].tolist() == [0]
    for k, (a, b) in enumerate(zip(got["acc"], alone["acc"])):
        assert np.array_equal(a[:-1], b[:-1]) and a[-2] == 1 and (a[-1], b[-1]) == (18, 0), k


# ---- batches under auto ------------------------------------------------------------------------------------------------------------
def test_the_random_batch_under_auto():
    """Seed 24, L from 1 .. 40 (the batch test_gpu_hmm_align_shapes.py documents): 5 of the 40 streams take 17 to 20 slots and lie
    between resident ones, so the launch is cut at every change of the body; every stream has status 0."""
    models, streams, transcripts, optionals = cases.random_batch(LC.RANDOM_SEED, LC.RANDOM_MAX_L)
    wide = [R.slots_of(models, u) > 16 for u in transcripts]
    assert sum(wide) == 5 and sum(a != b for a, b in zip(wide, wide[1:])) >= 4
    got, want = _run("auto", models, streams, transcripts, optionals, -1.0), _want(models, streams, transcripts, optionals, -1.0)
    _assert_equal(got, want, "auto")
    assert got["status"].tolist() == [0] * 40


def test_unlike_streams_and_a_seventeen_slot_stream_in_one_call():
    models, streams, transcripts, optionals = cases.unlike_streams()
    _m17, u17, s17 = cases.packing("64x17")
    # the 64-state classes 3 .. 5 stand in for the packing's three: the 17-slot stream goes between the resident ones
    streams = streams[:2] + [s17[:150]] + streams[2:]
    transcripts = transcripts[:2] + [u17 + 3] + transcripts[2:]
    optionals = optionals[:2] + [np.zeros(17, np.uint8)] + optionals[2:]
    assert [R.slots_of(models, u) for u in transcripts] == [1, 2, 17, 8, 3]
    got, want = _run("auto", models, streams, transcripts, optionals, -1.0), _want(models, streams, transcripts, optionals, -1.0)
    _assert_equal(got, want)
    assert got["status"].tolist() == [0] * 5
    with pytest.raises(Exception, match=r"stream 2: the units take 17 wave-slots"):
        _run("resident", models, streams, transcripts, optionals, -1.0)


# ---- the training loop -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epsilon", [1e-5, 0.0])
def test_two_iterations_under_auto_equal_the_restatements_on_the_bits(epsilon):
    models, units, stream = cases.packing("64x17")
    args = cases.pack([stream[:200], stream[200:300]], [units, units[:5]])
    assert hmm.embedded_estep(models, *args, -1.0, body="auto")["status"].tolist() == [0, 0]
    got, hist = hmm.train_embedded(models, *args, -1.0, epsilon, -1e300, 2, body="auto")
    want, whist = R.train(models, *args, -1.0, epsilon, -1e300, 2)
    assert len(hist) == 2 and np.array_equal(_bits(hist), _bits(np.array(whist)))
    for k, (g, w) in enumerate(zip(got, want)):
        for what, a, b in zip(("pi", "A", "B"), g, w):
            assert np.array_equal(_bits(a), _bits(b)), (k, what)
    assert not np.array_equal(got[0][2], models[0][2])


# ---- the file form -----------------------------------------------------------------------------------------------------------------
def test_the_file_form_trains_on_seventeen_labels_what_the_array_form_trains(tmp_path):
    models = cases.small_models(seed=17, Ns=(64, 2), zeros=0.0)
    for c, m in zip(("a", "bg"), models):
        hmm.save_model(tmp_path / f"{c}.hmm", c, *m)
    stream = np.random.default_rng(18).integers(0, M, 90).astype(np.uint16)
    e.formats.write_seq(str(tmp_path / "x.seq"), "_", M, stream)
    (tmp_path / "x.csv").write_text("class\n" + "a\n" * 17)
    units = np.array([1] + [0, 1] * 17, np.int32)  # the filler around and between the 17 labels
    opt = (units == 1).astype(np.uint8)
    assert R.slots_of(models, units) == 35
    want, whist = hmm.train_embedded(models, stream, [0, 90], units, [0, 35], opt, -1.0, 1e-5, -1e300, 2, body="auto")
    files = [str(tmp_path / "a.hmm"), str(tmp_path / "bg.hmm")]
    with pytest.raises(e.Ecoz2Error, match="the embedded E-step has no looped body"):
        hmm.learn_embedded_files(files, [str(tmp_path / "x.seq")], [str(tmp_path / "x.csv")], tmp_path / "no", -1.0, filler="bg")
    hmm.learn_embedded_files(files, [str(tmp_path / "x.seq")], [str(tmp_path / "x.csv")], tmp_path / "out", -1.0, filler="bg",
                             hmm_epsilon=1e-5, val_auto=-1e300, max_iterations=2, body="auto")
    for c, w in zip(("a", "bg"), want):
        g = hmm.load_model(tmp_path / "out" / f"{c}.hmm")
        assert all(np.array_equal(_bits(np.asarray(a)), _bits(b)) for a, b in zip(g[-3:], w)), c
    rows = (tmp_path / "out" / "embedded.csv").read_text().splitlines()
    assert len(whist) == 2 and rows[1:] == [f"{i},{'%.17g' % L},1,0" for i, L in enumerate(whist)]


# ---- the default -------------------------------------------------------------------------------------------------------------------
def test_with_nothing_set_seventeen_slots_are_still_refused():
    models, units, stream = cases.packing("64x17")
    with pytest.raises(Exception, match=r"stream 0: the units take 17 wave-slots of 64 lanes \(at most 16: the embedded E-step has no looped body\)"):
        _run(None, models, [stream], [units])
