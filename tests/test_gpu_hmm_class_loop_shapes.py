"""The four class-loop decoders on the GPU where their own files do not take them, on the inputs of
tests/hmm_class_loop_cases.py, every output against the numpy restatements on the bits (every array, the raw bits of every
double, the statuses; no tolerance): a symbol outside the alphabet and a symbol no state emits at the edges of the 64-symbol
hand-out, at the last frame, under both bodies and behind a chunk that is not the first; the same events in a session, at the
last symbol of a block, the first of the remainder and in what only close processes, fed whole, in two pieces and symbol by
symbol; class sets at the 4096 states the decoders admit (64 slots: four turns a looped wave, more than 64 KB of dynamic LDS,
live paths in all four states of a coalesce thread) and K = 1024 outside --class-transitions; seeded random sets through all
four decoders."""
import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_class_loop_cases as cases
from . import hmm_posterior_restatement as RP
from . import hmm_segment_restatement as R
from . import hmm_segment_stream_restatement as RS
from . import hmm_segment_trans_restatement as RT
from . import hmm_viterbi_restatement as V
from .test_gpu_hmm_posteriors import _assert_equal as _assert_post
from .test_gpu_hmm_segment import _assert_equal as _assert_seg
from .test_gpu_hmm_segment import _bits
from .test_gpu_hmm_segment_stream import _assert_one_shot, _same, _stream, block  # noqa: F401  (block: a fixture)
from .test_gpu_hmm_segment_trans import _assert_equal as _assert_trans

pytestmark = pytest.mark.gpu

NINF = float("-inf")


def _one(res, s, T=cases.EVENT_T, score="gbest"):
    """stream s of a batch of streams of T frames, as a call on that stream alone returns it"""
    out = {k: res[k][s * T:(s + 1) * T] for k in ("cls", "state", "entered", score)}
    out.update(log_prob=res["log_prob"][s:s + 1], status=res["status"][s:s + 1])
    return out


def _assert_segments(got, want, offs, ls):
    """`segments` as test_segment_equals_the_restatement builds them"""
    for s, segs in enumerate(got["segments"]):
        a, b = offs[s], offs[s + 1]
        ref = R.segments_of(want["cls"][a:b], want["entered"][a:b], want["gbest"][a:b], want["log_prob"][s], ls)
        assert [(g["begin"], g["end"], g["cls"]) for g in segs] == [r[:3] for r in ref]
        assert np.array_equal(_bits(np.array([g["log_prob"] for g in segs])), _bits(np.array([r[3] for r in ref])))


# ---- 1. events, the one-shot decoders --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def event_refs():
    """the restatements of the event batch, computed once: name -> dict (read only)"""
    streams, kinds = cases.event_batch()
    sym, offs = hmm._pack(streams)
    small = cases.event_models()
    ls = cases.EVENT_LN_SWITCH
    return dict(sym=sym, offs=offs, kinds=kinds, small=small, segment=R.segment(small, sym, offs, ls),
                trans=RT.segment_trans(small, sym, offs, cases.event_prices(3)), posteriors=RP.posteriors(small, sym, offs, ls))


# case: (the event models, ECOZ2_HMM_SEGMENT_BODY) -- the four instantiations of k_hmm_segment and of k_hmm_segment_stream:
# <false, true>, <true, true>, <false, false> (lA of six classes of 64 states stays in global memory), <true, false>
EVENT_CASES = {"resident": ("5_3_4", None), "forced_looped": ("5_3_4", "looped"), "resident_64x6": ("64x6", None),
               "looped_64x17": ("64x17", None)}


@pytest.mark.parametrize("case", list(EVENT_CASES))
def test_segment_meets_a_bad_and_a_dead_symbol_at_the_edges_of_the_hand_out(case, event_refs, monkeypatch):
    for k in ("ECOZ2_HMM_SEGMENT_BODY", "ECOZ2_HMM_SEGMENT_CHUNK_BYTES"):
        monkeypatch.delenv(k, raising=False)
    name, body = EVENT_CASES[case]
    if body:
        monkeypatch.setenv("ECOZ2_HMM_SEGMENT_BODY", body)
    ref = event_refs
    sym, offs, ls, T = ref["sym"], ref["offs"], cases.EVENT_LN_SWITCH, cases.EVENT_T
    models = cases.event_models(name)
    want = ref["segment"] if name == "5_3_4" else R.segment(models, sym, offs, ls)
    got = hmm.segment(models, sym, offs, ls)
    _assert_seg(got, want, case)
    assert got["status"].tolist() == [0] + [2] * 6 + [1] * 6 + [2, 2] * 3 == [cases.event_status(k, "segment") for k in ref["kinds"]]
    assert np.isfinite(got["log_prob"][0]) and (got["log_prob"][1:] == NINF).all()
    _assert_seg(hmm.segment(models, sym[:T], [0, T], ls), _one(got, 0), (case, "alone"))  # the clean stream alone: the same bits
    monkeypatch.setenv("ECOZ2_HMM_SEGMENT_CHUNK_BYTES", "1")  # one stream per launch: psi0 of an event stream is not 0
    _assert_seg(hmm.segment(models, sym, offs, ls), want, (case, "chunks"))


def test_segment_trans_meets_a_bad_and_a_dead_symbol_at_the_edges_of_the_hand_out(event_refs, monkeypatch):
    monkeypatch.delenv("ECOZ2_HMM_SEGMENT_CHUNK_BYTES", raising=False)
    ref = event_refs
    models, want, sym, offs, T = ref["small"], ref["trans"], ref["sym"], ref["offs"], cases.EVENT_T
    lt = cases.event_prices(3)
    got = hmm.segment_trans(models, sym, offs, lt)
    _assert_trans(got, want)
    assert got["status"].tolist() == [0] + [2] * 6 + [1] * 6 + [2, 2] * 3 == [cases.event_status(k, "trans") for k in ref["kinds"]]
    assert np.isfinite(got["log_prob"][0]) and (got["log_prob"][1:] == NINF).all()
    _assert_trans(hmm.segment_trans(models, sym[:T], [0, T], lt), _one(got, 0, score="exit_score"), "alone")
    monkeypatch.setenv("ECOZ2_HMM_SEGMENT_CHUNK_BYTES", "1")
    _assert_trans(hmm.segment_trans(models, sym, offs, lt), want, "chunks")


def test_the_posteriors_meet_a_bad_and_a_dead_symbol_at_the_edges_of_the_hand_out(event_refs, monkeypatch):
    monkeypatch.delenv("ECOZ2_HMM_POSTERIOR_CHUNK_BYTES", raising=False)
    ref = event_refs
    models, want, sym, offs, T, ls = ref["small"], ref["posteriors"], ref["sym"], ref["offs"], cases.EVENT_T, cases.EVENT_LN_SWITCH
    S = len(offs) - 1
    # A batch of clean streams goes first: memory the allocator hands out again then holds posteriors, not zeros, and a failed
    # stream's rows are +0.0 only if the kernel writes every one of them (T K = 390 entries by a workgroup of 64 threads).
    clean = hmm.segment_posteriors(models, np.tile(sym[:T], S), offs, ls)
    assert clean["status"].tolist() == [0] * S and (clean["post"].sum(axis=1) > 0.99).all()
    got = hmm.segment_posteriors(models, sym, offs, ls)
    _assert_post(got, want)
    # (the first event in frame order decides: (DEAD, M) is 1, (M, DEAD) is 2)
    assert got["status"].tolist() == [0] + [2] * 6 + [1] * 6 + [1, 2] * 3 == [cases.event_status(k, "posteriors") for k in ref["kinds"]]
    assert np.isfinite(got["log_prob"][0]) and (got["log_prob"][1:] == NINF).all()
    failed = got["post"][T:]
    assert failed.shape == ((S - 1) * T, 3) and not failed.any() and not np.signbit(failed).any()
    alone = hmm.segment_posteriors(models, sym[:T], [0, T], ls)
    _assert_post(alone, dict(post=got["post"][:T], log_prob=got["log_prob"][:1], status=got["status"][:1]), "alone")
    assert np.array_equal(_bits(clean["post"][:T]), _bits(alone["post"]))
    monkeypatch.setenv("ECOZ2_HMM_POSTERIOR_CHUNK_BYTES", "1")  # one stream per launch: a0 of an event stream is not 0
    _assert_post(hmm.segment_posteriors(models, sym, offs, ls), want, "chunks")


# ---- 2. events, the session ------------------------------------------------------------------------------------------------------
def _session_log(models, seq, ls, feeds):
    """cases.session_script, by the library: the same entries from hmm.SegmentStream"""
    log, at = [], 0
    with hmm.SegmentStream(models, ls) as s:
        for n in feeds:
            bad = None
            try:
                out = s.feed(seq[at:at + n])
            except e.Ecoz2Error as err:
                msg = str(err)
                assert "is outside the models' alphabet of %d; the session takes no more symbols" % cases.EVENT_M in msg, msg
                out, bad = None, int(msg.split("the symbol at frame ")[1].split()[0])
            at += n
            log.append(dict(out=out, final=s.final_frames, bad_frame=bad))
            if bad is not None:
                with pytest.raises(e.Ecoz2Error) as ei:  # (the restatement asserts here)
                    s.feed(seq[:1])
                assert "takes no more symbols" in str(ei.value)
                break
        out = s.close()
        log.append(dict(out=out, final=s.final_frames, bad_frame=None, status=s.status, log_prob=s.log_prob))
    return log


def _assert_same_log(got, want, note):
    assert len(got) == len(want), note
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g["final"], g["bad_frame"]) == (w["final"], w["bad_frame"]), (note, i)
        assert (g["out"] is None) == (w["out"] is None), (note, i)
        if g["out"] is not None:
            n = len(w["out"]["cls"])
            assert len(g["out"]["cls"]) == n and (n == 0 or g["out"]["first"] == w["out"]["first"]), (note, i)
            for k, dt in (("cls", np.uint16), ("state", np.uint16), ("entered", np.uint8), ("gbest", np.float64)):
                assert _same(g["out"][k], np.array(w["out"][k], dtype=dt)), (note, i, k)
    assert got[-1]["status"] == want[-1]["status"] and _bits(np.float64(got[-1]["log_prob"])) == _bits(np.float64(want[-1]["log_prob"])), note
    assert got[-1]["final"] == want[-1]["fed"], note


SESSION_FEEDS = {"whole": [130], "64_66": [64, 66], "single": [1] * 130}


@pytest.mark.parametrize("case", list(EVENT_CASES))
def test_a_session_meets_a_bad_symbol_at_the_edges_of_the_hand_out_and_of_the_block(case, block, monkeypatch):
    """everything the session returns or raises is what hmm_segment_stream_restatement.Stream does with the same feeds"""
    block(cases.EVENT_SESSION_B)
    name, body = EVENT_CASES[case]
    if body:
        monkeypatch.setenv("ECOZ2_HMM_SEGMENT_BODY", body)
    models = cases.event_models(name)
    lms = [V.log_model(*m) for m in models]
    clean = cases.event_batch()[0][0]
    ls, B = cases.EVENT_LN_SWITCH, cases.EVENT_SESSION_B
    for p in cases.SESSION_BAD_AT:
        seq = cases.with_symbols(clean, {p: cases.EVENT_M})
        for fname, feeds in SESSION_FEEDS.items():
            want = cases.session_script(lms, seq, ls, B, feeds)
            got = _session_log(models, seq, ls, feeds)
            _assert_same_log(got, want, (case, p, fname))
            assert got[-1]["status"] == 2 and got[-1]["log_prob"] == NINF
            assert [g["bad_frame"] for g in got if g["bad_frame"] is not None] == ([p] if p < B else [])


@pytest.mark.parametrize("case", list(EVENT_CASES))
def test_a_session_over_a_stream_that_dies_is_the_one_shot_decode(case, block, monkeypatch):
    block(cases.EVENT_SESSION_B)
    ename, body = EVENT_CASES[case]
    if body:
        monkeypatch.setenv("ECOZ2_HMM_SEGMENT_BODY", body)
    models = cases.event_models(ename)
    lms = [V.log_model(*m) for m in models]
    clean = cases.event_batch()[0][0]
    ls, B, T = cases.EVENT_LN_SWITCH, cases.EVENT_SESSION_B, cases.EVENT_T
    for p in cases.SESSION_DEAD_AT:
        seq = cases.with_symbols(clean, {p: cases.DEAD})
        one = R.segment(models, seq, [0, T], ls)
        assert one["status"].tolist() == [1]
        for name, feeds in SESSION_FEEDS.items():
            rest, finals = RS.decode(lms, seq, ls, B, feeds)
            got = _stream(models, seq, ls, feeds)
            _assert_one_shot(got, one, (case, p, name))  # status 1, every frame, by the rules of a stream that lives
            assert got["finals"] == finals and got["status"] == rest.status == 1 and got["total"] == T
            assert (got["cls"].tolist(), got["state"].tolist(), got["entered"].tolist()) == (rest.cls, rest.state, rest.entered)
            assert _same(got["gbest"], np.array(rest.gbest))
    # a dead stream that meets a bad symbol in what close processes
    seq = cases.with_symbols(clean, {63: cases.DEAD, 110: cases.EVENT_M})
    for name, feeds in SESSION_FEEDS.items():
        _assert_same_log(_session_log(models, seq, ls, feeds), cases.session_script(lms, seq, ls, B, feeds), (case, "dead_then_bad", name))


# ---- 3. the rows of SHAPES -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.SHAPES))
def test_segment_equals_the_restatement_at_every_row(name, monkeypatch):
    for k in ("ECOZ2_HMM_SEGMENT_BODY", "ECOZ2_HMM_SEGMENT_CHUNK_BYTES"):
        monkeypatch.delenv(k, raising=False)
    models, stream = cases.shape(name)
    T, ls = len(stream), cases.LN_SWITCH
    ref = cases.shape_reference(name)
    want = dict(ref, log_prob=np.array([ref["log_prob"]]), status=np.array([ref["status"]], dtype=np.int32))
    got = hmm.segment(models, stream, [0, T], ls)
    _assert_seg(got, want, name)
    _assert_segments(got, want, [0, T], ls)
    assert got["status"].tolist() == [0] and len(got["segments"][0]) >= 10


@pytest.mark.parametrize("name", ["1x1024", "40_1x24_x14"])
def test_the_posteriors_equal_the_restatement_at_the_wide_rows(name, monkeypatch):
    monkeypatch.delenv("ECOZ2_HMM_POSTERIOR_CHUNK_BYTES", raising=False)
    models, stream = cases.shape(name)
    T = len(stream)
    got = hmm.segment_posteriors(models, stream, [0, T], cases.LN_SWITCH)
    _assert_post(got, RP.posteriors(models, stream, [0, T], cases.LN_SWITCH), name)
    assert got["status"].tolist() == [0] and got["post"].shape == (T, len(models))


def test_segment_trans_of_1024_leaning_classes_equals_the_restatement(monkeypatch):
    monkeypatch.delenv("ECOZ2_HMM_SEGMENT_CHUNK_BYTES", raising=False)
    models, stream = cases.shape("1x1024")
    T = len(stream)
    lt = cases.forbidding_prices(1024, len(models))  # a fifth of the moves is forbidden
    assert 0.15 < np.mean(lt == NINF) < 0.25
    got = hmm.segment_trans(models, stream, [0, T], lt)
    want = RT.segment_trans(models, stream, [0, T], lt)
    _assert_trans(got, want, "1x1024")
    assert got["status"].tolist() == [0] and got["entered"].sum() >= 10


@pytest.mark.parametrize("pattern", ["whole", "whole_blocks", "63_64_65"])  # ("whole" walks back once, from frame 191 alone)
@pytest.mark.parametrize("name", cases.SESSION_SHAPES)
def test_a_session_over_the_row_is_the_one_shot_restatement(name, pattern, block):
    block(cases.SESSION_B)
    models, stream = cases.shape(name)
    T, ls = len(stream), cases.LN_SWITCH
    ref = cases.shape_reference(name)
    want = dict(ref, log_prob=np.array([ref["log_prob"]]), status=np.array([ref["status"]], dtype=np.int32))
    rest, finals = cases.session_reference(name, pattern)
    got = _stream(models, stream, ls, cases.session_feeds(T, pattern))
    _assert_one_shot(got, want, (name, pattern))
    assert got["finals"] == finals and got["stats"]["peak_pending"] == rest.peak_pending
    assert finals[-1] > 0  # (frames were decided by k_hmm_segment_coalesce, not at close alone)


# ---- 4. the random sets ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_all():
    return cases.random_sets(cases.RANDOM_SEED)


@pytest.fixture(scope="module")
def random_resident():
    return cases.random_sets(cases.RANDOM_SEED, resident_only=True)


def test_segment_on_the_random_sets(random_all, monkeypatch):
    for k in ("ECOZ2_HMM_SEGMENT_BODY", "ECOZ2_HMM_SEGMENT_CHUNK_BYTES"):
        monkeypatch.delenv(k, raising=False)
    for i, row in enumerate(random_all):
        sym, offs = hmm._pack(row["streams"])
        got = hmm.segment(row["models"], sym, offs, row["ln_switch"])
        want = R.segment(row["models"], sym, offs, row["ln_switch"])
        _assert_seg(got, want, (i, row["Ns"]))
        _assert_segments(got, want, offs, row["ln_switch"])


def test_a_session_on_the_random_sets(random_all, block):
    block(cases.SESSION_B)
    for i, row in enumerate(random_all):
        lms = [V.log_model(*m) for m in row["models"]]
        for j, seq in enumerate(row["streams"]):
            T = len(seq)
            feeds = [50] * (T // 50) + [T % 50]
            rest, finals = RS.decode(lms, seq, row["ln_switch"], cases.SESSION_B, feeds)
            want = R.segment(row["models"], seq, [0, T], row["ln_switch"])
            got = _stream(row["models"], seq, row["ln_switch"], feeds)
            _assert_one_shot(got, want, (i, j))
            assert got["finals"] == finals and got["stats"]["peak_pending"] == rest.peak_pending, (i, j)


@pytest.mark.parametrize("i", range(12))  # (a case per set: the restatement of the twelve takes eight seconds)
def test_the_posteriors_on_the_random_sets(i, random_resident, monkeypatch):
    monkeypatch.delenv("ECOZ2_HMM_POSTERIOR_CHUNK_BYTES", raising=False)
    row = random_resident[i]
    sym, offs = hmm._pack(row["streams"])
    got = hmm.segment_posteriors(row["models"], sym, offs, row["ln_switch"])
    _assert_post(got, RP.posteriors(row["models"], sym, offs, row["ln_switch"]), (i, row["Ns"]))


def test_segment_trans_on_the_random_sets_and_the_uniform_matrix(random_resident, monkeypatch):
    for k in ("ECOZ2_HMM_SEGMENT_BODY", "ECOZ2_HMM_SEGMENT_CHUNK_BYTES"):
        monkeypatch.delenv(k, raising=False)
    for i, row in enumerate(random_resident):
        K = len(row["Ns"])
        sym, offs = hmm._pack(row["streams"])
        lt = cases.forbidding_prices(i, K)
        _assert_trans(hmm.segment_trans(row["models"], sym, offs, lt), RT.segment_trans(row["models"], sym, offs, lt), (i, row["Ns"]))
        # every price equal to ln_switch: the path and ln P* of `hmm segment` (the equivalence of 4.8.8, at random shapes)
        uni = hmm.segment_trans(row["models"], sym, offs, np.full((K, K), row["ln_switch"]))
        ref = hmm.segment(row["models"], sym, offs, row["ln_switch"])
        _assert_trans(uni, ref, (i, "uniform"), keys=("cls", "state", "entered", "log_prob", "status"))
