"""The looped body of `hmm segment --class-transitions` and of its session on the GPU (DESIGN.md 4.8.8 and 4.8.15,
ECOZ2_HMM_SEGMENT_TRANS_BODY): above 16 wave-slots cls, state, entered, the raw bits of exit_score and ln P*, status and the
segments against the numpy restatements, which have no slot cap; below the cap the looped body forced against the resident one
at every (lA, lt) placement; ties and forbidden moves across a wave's turns; every status; a small table budget; one price
everywhere against `hmm segment`; the session against the one-shot decode, against its restatement feed by feed and against
the resident session call by call; the files and the CLI; what still refuses 17 slots.  No tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_segment_trans_cases as cases
from . import hmm_segment_trans_looped_cases as LC
from . import hmm_segment_trans_restatement as RT
from . import hmm_segment_trans_stream_restatement as ST
from . import hmm_viterbi_restatement as V
from .test_gpu_hmm_segment_trans import SHAPES as BELOW_SHAPES
from .test_gpu_hmm_segment_trans import _init_models, _streams

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
NINF = float("-inf")
KEYS = LC.KEYS
FRAME_KEYS = ("cls", "state", "entered", "exit_score")
SLOTS17 = "the classes take 17 wave-slots of 64 lanes (at most 16: the class-transition decoder has no looped body)"
SLOTS17_POST = "the classes take 17 wave-slots of 64 lanes (at most 16: the posteriors under class-to-class prices have no looped body)"


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in (LC.BODY, LC.CHUNK, LC.ENV_BLOCK, LC.ENV_PENDING, "ECOZ2_HMM_SEGMENT_BODY"):
        monkeypatch.delenv(k, raising=False)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _assert_equal(got, want, note=None, keys=KEYS):
    for key in keys:
        a, b = _bits(got[key]), _bits(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (key, note, np.flatnonzero(a != b)[:5] if a.shape == b.shape else (a.shape, b.shape))
    if "segments" in want:
        assert got["segments"] == want["segments"], note


def _assert_segments(got, want, offs, lt, note=None):
    """the mirror's segments against the restatement's host arithmetic, begin / end / class exact and log_prob by its bits"""
    for s, segs in enumerate(got["segments"]):
        a, b = offs[s], offs[s + 1]
        ref = RT.segments_of(want["cls"][a:b], want["entered"][a:b], want["exit_score"][a:b], want["log_prob"][s], lt)
        assert [(g["begin"], g["end"], g["cls"]) for g in segs] == [r[:3] for r in ref], note
        assert np.array_equal(_bits(np.array([g["log_prob"] for g in segs], dtype=np.float64)),
                              _bits(np.array([r[3] for r in ref], dtype=np.float64))), note


def _against_the_restatement(models, sym, offs, lt, body, note=None):
    got = hmm.segment_trans(models, sym, offs, lt, body=body)
    want = RT.segment_trans(models, sym, offs, lt)
    _assert_equal(got, want, (note, body))
    _assert_segments(got, want, offs, lt, (note, body))
    return got


# ---- 1. every wide row ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LC.WIDE))
def test_the_wide_rows_equal_the_restatement_under_auto_and_looped(name):
    models, stream, lt = LC.wide_case(name)
    offs = np.array([0, len(stream)], dtype=np.int64)
    want = LC.wide_reference(name)
    for body in ("auto", "looped"):
        got = hmm.segment_trans(models, stream, offs, lt, body=body)
        _assert_equal(got, want, (name, body))
        _assert_segments(got, want, offs, lt, (name, body))
        assert len(got["segments"][0]) == int(np.sum(want["entered"])) >= 2
        assert hmm.segment_trans_last_kernel_ms() > 0.0


# ---- 2. stream lengths around the resident body's hand-out ------------------------------------------------------------------------
def test_lengths_around_the_hand_out_and_an_empty_stream_in_one_call():
    Ns, M = (64,) * 20, 32
    models = LC.loop_cases.leaning_models(LC.MODEL_SEED, Ns, M)
    lengths = (1, 2, 63, 0, 64, 65, 129)
    sym, offs = hmm._pack([LC.loop_cases.run_stream(20 + i, len(Ns), M, T) for i, T in enumerate(lengths)])
    lt = LC.loop_cases.forbidding_prices(LC.PRICE_SEED, len(Ns))
    for body in ("auto", "looped"):
        got = _against_the_restatement(models, sym, offs, lt, body, lengths)
        assert got["status"].tolist() == [0] * 7 and got["log_prob"][3] == 0.0


# ---- 3. the looped body forced below the cap -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.BELOW_THE_CAP)
def test_below_the_cap_the_looped_body_equals_the_resident_one(name):
    Ns, M, lengths = BELOW_SHAPES[name]
    models = _init_models(Ns, M)
    rng = np.random.default_rng(len(Ns) + M)
    sym, offs = hmm._pack(_streams(rng, M, lengths))
    lt = cases.random_prices(rng, len(Ns))
    resident = hmm.segment_trans(models, sym, offs, lt, body="resident")
    looped = hmm.segment_trans(models, sym, offs, lt, body="looped")
    _assert_equal(looped, resident, name)
    _assert_equal(hmm.segment_trans(models, sym, offs, lt, body="auto"), resident, name)
    _assert_equal(hmm.segment_trans(models, sym, offs, lt), resident, name)
    assert resident["status"].tolist() == [0] * len(lengths)


# ---- 4. ties and forbidden moves across the turns ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mtype", [1, 2, 3])  # uniform (every comparison a tie), cascades (-inf in pi and A)
@pytest.mark.parametrize("name", ["64x17", "5x204"])
def test_ties_and_forbidden_moves_inside_the_models(name, mtype):
    Ns = LC.WIDE[name][0]
    M, K = 8, len(Ns)
    models = _init_models(Ns, M, mtype)
    rng = np.random.default_rng(mtype)
    sym, offs = hmm._pack(_streams(rng, M, (1, 40, 65)))
    for lt in (cases.random_prices(rng, K), np.full((K, K), NINF), np.zeros((K, K))):
        _against_the_restatement(models, sym, offs, lt, "auto", (name, mtype))


def test_a_copy_in_slot_16_of_the_class_in_slot_0_loses_every_tie():
    """wave 0 serves both, in different turns; the copy pays what its original pays, so every maximum that class 0 reaches is
    reached by class 16 as well, and the lower class must win"""
    Ns, M, _T = LC.WIDE["64x17"]
    models = list(LC.loop_cases.leaning_models(LC.MODEL_SEED, Ns, M))
    models[16] = models[0]
    dup = list(range(16)) + [0]
    rng = np.random.default_rng(6)
    small = cases.random_prices(rng, 16, forbidden=0.0) / 20.0  # (cheap enough that the paths do switch)
    lt = small[np.ix_(dup, dup)]
    streams = [LC.loop_cases.run_stream(30 + i, 16, M, T) for i, T in enumerate((1, 2, 64, 200))]  # (the symbols of classes 0 .. 15)
    sym, offs = hmm._pack(streams)
    got = _against_the_restatement(models, sym, offs, lt, "auto")
    visited = set(int(k) for k in got["cls"])
    assert 0 in visited and 16 not in visited and len(visited) > 4


# ---- 5. every status in one call ---------------------------------------------------------------------------------------------------
def test_streams_of_every_status_in_one_call_at_seventeen_slots():
    e.hmm.set_random_seed(5)
    M = 8
    models = []
    for _k in range(17):
        pi, A, B = hmm.init_model(64, M, 3)
        B[:, 5] = 0.0  # symbol 5 cannot be emitted by any state of any class
        models.append((pi, A, B))
    rng = np.random.default_rng(2)
    good = lambda T: rng.integers(0, 5, T).astype(np.uint16)
    bad = lambda T, at: LC.loop_cases.with_symbols(good(T), {at: M + 1})
    seqs = [good(70), np.zeros(0, dtype=np.uint16), bad(70, 0), bad(70, 63), bad(70, 64), LC.loop_cases.with_symbols(good(70), {33: 5}), good(3)]
    sym, offs = hmm._pack(seqs)
    lt = cases.random_prices(np.random.default_rng(1), 17)
    got = _against_the_restatement(models, sym, offs, lt, "auto")  # (status 1 still writes the path, by the same rules)
    assert got["status"].tolist() == [0, 0, 2, 2, 2, 1, 0]
    assert got["log_prob"][1] == 0.0 and got["log_prob"][2:6].tolist() == [NINF] * 4 and np.isfinite(got["log_prob"][[0, 6]]).all()
    for s in (2, 3, 4):
        a, b = offs[s], offs[s + 1]
        assert got["cls"][a:b].tolist() == [0xFFFF] * 70 and got["exit_score"][a:b].tolist() == [0.0] + [NINF] * 69


# ---- 6. a small table budget -------------------------------------------------------------------------------------------------------
def test_a_small_table_budget_gives_the_same_bits(monkeypatch):
    Ns, M, _T = LC.WIDE["33x20"]
    models, _stream, lt = LC.wide_case("33x20")
    rng = np.random.default_rng(4)
    sym, offs = hmm._pack([LC.loop_cases.run_stream(40 + i, len(Ns), M, int(T)) for i, T in enumerate(rng.integers(0, 60, 12))])
    one = _against_the_restatement(models, sym, offs, lt, "auto")
    for budget in ("1", str((2 * sum(Ns) + 12 * len(Ns)) * 100)):  # one stream per launch; a few streams per launch
        monkeypatch.setenv(LC.CHUNK, budget)
        _assert_equal(hmm.segment_trans(models, sym, offs, lt, body="auto"), one, budget)


# ---- 7. one price everywhere is hmm segment ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["64x17", "33x20"])
def test_one_price_everywhere_is_hmm_segment(name):
    models, stream, _lt = LC.wide_case(name)
    K, offs = len(models), [0, len(stream)]
    got = hmm.segment_trans(models, stream, offs, np.full((K, K), cases.UNIFORM_PRICE), body="auto")
    ref = hmm.segment(models, stream, offs, cases.UNIFORM_PRICE)  # (its own looped body: more than 16 slots)
    _assert_equal(got, ref, name, keys=("cls", "state", "entered", "log_prob", "status"))
    at = np.flatnonzero(ref["entered"])
    assert len(at) >= 2 and np.array_equal(_bits(got["exit_score"][at]), _bits(ref["gbest"][at]))


# ---- 8. the session ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def block(monkeypatch):
    monkeypatch.setenv(LC.ENV_BLOCK, str(LC.SESSION_B))
    monkeypatch.setenv(LC.ENV_PENDING, str(16 << 20))


def _session(models, sym, lt, feeds, body):
    """the session fed sym in pieces of the lengths `feeds`, then closed -> (the dict of each call, the close last; final frames
    after each feed; log_prob; status)"""
    parts, finals, at = [], [], 0
    with hmm.SegmentTransStream(models, lt, body=body) as s:
        assert LC.BODY not in os.environ  # (the variable is set around open only: the session has fixed its body)
        for n in feeds:
            parts.append(s.feed(sym[at:at + n]))
            at += n
            finals.append(s.final_frames)
        assert at == len(sym)
        parts.append(s.close())
        assert s.final_frames == len(sym) and (len(sym) == 0 or s.kernel_ms() > 0.0)
        return parts, finals, s.log_prob, s.status


def _joined(parts):
    at = 0
    for p in parts:  # (the frames come in order, each once)
        assert p["first"] == at or len(p["cls"]) == 0
        at += len(p["cls"])
    out = {k: np.concatenate([p[k] for p in parts]) for k in FRAME_KEYS}
    out["segments"] = [g for p in parts for g in p["segments"]]
    return out


@pytest.mark.parametrize("pattern", ["whole", "whole_blocks", "63_64_65"])
@pytest.mark.parametrize("name", LC.SESSION_ROWS)
def test_the_session_equals_the_one_shot_decode_and_its_restatement(name, pattern, block):
    models, stream, lt = LC.wide_case(name)
    T = len(stream)
    feeds = LC.loop_cases.session_feeds(T, pattern)
    parts, finals, lp, status = _session(models, stream, lt, feeds, "auto")
    got = _joined(parts)
    want = hmm.segment_trans(models, stream, [0, T], lt, body="auto")
    _assert_equal(want, LC.wide_reference(name), name)
    for k in FRAME_KEYS:
        assert _same(got[k], want[k]), (name, pattern, k)
    assert _bits(np.float64(lp)) == _bits(want["log_prob"])[0] and status == want["status"][0] == 0
    assert got["segments"] == want["segments"][0]
    # what is final after each feed, and the frames themselves, are the restatement's
    rest, rest_finals = LC.session_reference(name, pattern)
    assert rest.join_failures == 0 and finals == rest_finals
    assert got["cls"].tolist() == rest.cls and got["state"].tolist() == rest.state and got["entered"].tolist() == rest.entered
    assert _same(got["exit_score"], np.array(rest.exit_score, dtype=np.float64))
    assert _bits(np.float64(lp)) == _bits(np.float64(rest.log_prob)) and status == rest.status
    at = 0
    for n, p, fin in zip(feeds, parts, finals):  # each call hands out exactly the frames that became final in it
        assert len(p["cls"]) == fin - at
        at = fin


@pytest.mark.parametrize("name", ["5x12", "mixed"])
def test_below_the_cap_the_looped_session_equals_the_resident_one_call_by_call(name, block):
    Ns, M, _lengths = BELOW_SHAPES[name]
    models = LC.loop_cases.leaning_models(LC.MODEL_SEED, Ns, M)
    lt = LC.loop_cases.forbidding_prices(LC.PRICE_SEED, len(Ns), 0.0)
    stream = LC.loop_cases.run_stream(LC.STREAM_SEED, len(Ns), M, 200)
    for pattern in ("whole", "whole_blocks", "63_64_65"):
        feeds = LC.loop_cases.session_feeds(len(stream), pattern)
        a = _session(models, stream, lt, feeds, "looped")
        b = _session(models, stream, lt, feeds, "resident")
        assert a[1] == b[1] and a[3] == b[3] == 0 and _bits(np.float64(a[2])) == _bits(np.float64(b[2]))
        assert len(a[0]) == len(b[0])
        for pa, pb in zip(a[0], b[0]):
            assert pa["first"] == pb["first"] and pa["segments"] == pb["segments"]
            for k in FRAME_KEYS:
                assert _same(pa[k], pb[k]), (name, pattern, k)
        assert any(fin > 0 for fin in a[1][:-1]) or pattern == "whole"  # (something is decided before close)
        one = hmm.segment_trans(models, stream, [0, len(stream)], lt, body="looped")
        for k in FRAME_KEYS:
            assert _same(_joined(a[0])[k], one[k]), (name, pattern, k)


def _dead_session(models, lms, sym, lt, feeds, body):
    """the same feeds to the session and to the restatement's Stream; a refused feed ends the feeding -> (frames, status, ln P*, rest)"""
    rest = ST.Stream(lms, lt, LC.SESSION_B)
    parts, at = [], 0
    with hmm.SegmentTransStream(models, lt, body=body) as s:
        for n in feeds:
            piece = sym[at:at + n]
            at += n
            bad = None
            try:
                rest.feed(piece)
            except ST.BadSymbol as ex:
                bad = ex.frame
            if bad is None:
                parts.append(s.feed(piece))
            else:
                with pytest.raises(e.Ecoz2Error) as ei:
                    s.feed(piece)
                assert f"the symbol at frame {bad} is outside the models' alphabet" in str(ei.value)
                with pytest.raises(e.Ecoz2Error):  # dead: it takes no more symbols
                    s.feed(piece)
            assert s.final_frames == rest.F
            if bad is not None:
                break
        rest.close()
        parts.append(s.close())
        got = {k: np.concatenate([p[k] for p in parts]) for k in FRAME_KEYS}
        return got, s.status, s.log_prob, s.final_frames, rest


@pytest.mark.parametrize("at", [63, 64, 99, 100])
def test_a_symbol_outside_the_alphabet_leaves_the_session_dead_as_the_resident_one_is(at, block):
    M, T = 8, 130
    feeds = {"whole": [T], "blocks": [64, 64, 2], "63_64_3": [63, 64, 3]}
    for Ns, bodies in (([5] * 13, ("looped", "resident")), ([64] * 17, ("auto",))):
        K = len(Ns)
        models = _init_models(Ns, M)
        lms = [V.log_model(*m) for m in models]
        rng = np.random.default_rng(6)
        lt = cases.random_prices(rng, K, 0.2)
        sym = rng.integers(0, M, T).astype(np.uint16)
        sym[at] = M
        for pname, fd in feeds.items():
            outs = []
            for body in bodies:
                got, status, lp, total, rest = _dead_session(models, lms, sym, lt, fd, body)
                assert (status, lp, rest.status, rest.log_prob) == (2, NINF, 2, NINF), (K, pname, body)
                assert total == rest.F == len(got["cls"])
                assert got["cls"].tolist() == rest.cls and got["state"].tolist() == rest.state and got["entered"].tolist() == rest.entered
                assert _same(got["exit_score"], np.array(rest.exit_score, dtype=np.float64)), (K, pname, body)
                assert got["cls"][at:].tolist() == [0xFFFF] * (total - at)  # (no frame from the bad one on is ever final)
                outs.append(got)
            for k in FRAME_KEYS:
                assert all(_same(o[k], outs[0][k]) for o in outs[1:])


# ---- 9. files and the CLI ------------------------------------------------------------------------------------------------------------
def test_files_and_the_cli_at_seventeen_models_of_64_states(tmp_path, capfd):
    env = dict(os.environ)
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_GPUS", "ECOZ2_HMM_SEGMENT_BODY", LC.BODY, LC.CHUNK, LC.ENV_PENDING):
        env.pop(k, None)
    env[LC.ENV_BLOCK] = str(LC.SESSION_B)
    W_ms, O_ms, ls = 45, 15, -2.0
    models, sym, file_lt = LC.wide_case("64x17")
    M = LC.WIDE["64x17"][1]
    names = [f"c{k:02d}" for k in range(17)]  # (the order in which a directory of models is resolved)
    for c, m in zip(names, models):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)
    hmm.write_class_transitions(tmp_path / "t.csv", names, file_lt)
    cuts = [0, 70, 71, len(sym)]  # (a piece of one frame among them)
    (tmp_path / "seq").mkdir()
    for i in range(3):
        e.formats.write_seq(str(tmp_path / "seq" / f"p{i}.seq"), "_", M, sym[cuts[i]:cuts[i + 1]])
    e.formats.write_seq(str(tmp_path / "cat.seq"), "_", M, sym)
    pieces = [f"seq/p{i}.seq" for i in range(3)]

    def run(*args):
        return subprocess.run([EXE, "hmm", "segment", "--models", "hmms", "--switch-penalty", str(ls), "--class-transitions", "t.csv", *args],
                              cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)

    r = run("--sequences", "cat.seq", "-c", "one", "--grammar-body", "auto")
    assert r.returncode == 0, (r.stdout, r.stderr)
    want = (tmp_path / "one" / "cat.csv").read_bytes()
    # the CSV that the array call implies
    lt = file_lt + ls
    got = hmm.segment_trans(models, sym, [0, len(sym)], lt, body="auto")
    _assert_equal(got, RT.segment_trans(models, sym, [0, len(sym)], lt))
    names_c, _k = hmm._strs(names)
    capfd.readouterr()
    assert e.lib.e2vq_hmm_segment_trans_report(b"cat.seq", len(sym), 17, names_c, W_ms, O_ms, got["cls"].ctypes.data,
                                               got["entered"].ctypes.data, got["exit_score"].ctypes.data, float(got["log_prob"][0]),
                                               ls, np.ascontiguousarray(lt).ctypes.data, str(tmp_path / "arr.csv").encode()) == 0
    capfd.readouterr()
    assert (tmp_path / "arr.csv").read_bytes() == want and want.count(b"\n") == len(got["segments"][0]) + 1 >= 3
    # the pieces as one stream are the concatenated file byte for byte
    r = run("--sequences", *pieces, "-c", "cont", "--grammar-continuous", "rec", "--grammar-body", "auto")
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert (tmp_path / "cont" / "rec.csv").read_bytes() == want and sorted(os.listdir(tmp_path / "cont")) == ["rec.csv"]
    # the Python mirrors of both file forms
    hmm_files = [str(tmp_path / "hmms" / f"{c}.hmm") for c in names]
    hmm.segment_files(hmm_files, [str(tmp_path / "cat.seq")], ls, csv=tmp_path / "py", class_transitions=tmp_path / "t.csv", grammar_body="auto")
    assert (tmp_path / "py" / "cat.csv").read_bytes() == want
    os.environ[LC.ENV_BLOCK] = str(LC.SESSION_B)
    try:
        hmm.segment_files(hmm_files, [str(tmp_path / p) for p in pieces], ls, csv=tmp_path / "pyc" / "x.csv", class_transitions=tmp_path / "t.csv",
                          grammar_continuous="rec", grammar_body="looped")
    finally:
        del os.environ[LC.ENV_BLOCK]
    assert (tmp_path / "pyc" / "x.csv").read_bytes() == want
    # without the flag, and with `resident`: the old refusal word for word, status 1, and nothing is written
    for extra in ([], ["--grammar-body", "resident"]):
        for mode in (["--sequences", "cat.seq"], ["--sequences", *pieces, "--grammar-continuous", "rec"]):
            r = run(*mode, "-c", "refused", *extra)
            assert r.returncode == 1 and SLOTS17 in r.stdout, (r.stdout, r.stderr)
            assert not (tmp_path / "refused").exists()


# ---- 10. what still refuses 17 slots ---------------------------------------------------------------------------------------------------
def test_seventeen_slots_are_still_refused_without_the_opt_in_and_by_the_posteriors(monkeypatch):
    models = _init_models([64] * 17, 4)
    sym, lt = np.zeros(4, np.uint16), np.zeros((17, 17))
    for kw in ({}, dict(body="resident")):
        with pytest.raises(e.Ecoz2Error) as ei:
            hmm.segment_trans(models, sym, [0, 4], lt, **kw)
        assert "e2vq_hmm_segment_trans: " + SLOTS17 in str(ei.value)
        with pytest.raises(e.Ecoz2Error) as ei:
            hmm.SegmentTransStream(models, lt, **kw)
        assert "e2vq_hmm_segment_trans_stream_open: " + SLOTS17 in str(ei.value)
    monkeypatch.setenv(LC.BODY, "auto")
    assert hmm.segment_trans(models, sym, [0, 4], lt)["status"].tolist() == [0]  # (the variable alone opts in)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment_trans_posteriors(models, sym, [0, 4], lt)
    assert "e2vq_hmm_segment_trans_posteriors: " + SLOTS17_POST in str(ei.value)
