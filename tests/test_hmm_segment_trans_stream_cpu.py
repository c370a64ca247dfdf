"""`hmm segment --class-transitions --grammar-continuous`, CPU side: the streaming restatement under a
matrix of prices against `segment_trans_logs` / `transcribe` on the concatenation for every block length and feed pattern; on
the planted stream, that frames are decided long before the end (and never where no price is finite); the refusals of
e2vq_hmm_segment_trans_stream_open, of e2vq_hmm_segment_trans_continuous_files and of the CLI, which come before any HIP
call; the exports and the usage text; the kernels' compiler metadata.  The GPU tests are in
test_gpu_hmm_segment_trans_stream.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_segment_restatement as R1
from . import hmm_segment_trans_cases as cases
from . import hmm_segment_trans_restatement as RT
from . import hmm_segment_trans_stream_restatement as ST
from . import hmm_viterbi_restatement as V
from .test_hmm_segment_stream_cpu import feed_patterns, planted_models, planted_stream, random_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXE = os.path.join(CSRC, "ecoz2")
NINF = float("-inf")
ENV_BLOCK = "ECOZ2_HMM_SEGMENT_STREAM_BLOCK"
ENV_PENDING = "ECOZ2_HMM_SEGMENT_STREAM_PENDING_BYTES"


def _err():
    return e.lib.e2vq_last_error().decode()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _uniform(N, M):
    return np.full(N, 1.0 / N), np.full((N, N), 1.0 / N), np.full((N, M), 1.0 / M)


def planted_prices(kind="cycle"):
    """log P - 5.  cycle: P[f][(f + 1) mod 3] = 0.9 and 0.05 elsewhere; no_diagonal: the same with the diagonal forbidden;
    reverse: the cycle the other way round"""
    P = np.full((3, 3), 0.05)
    for f in range(3):
        P[f][(f + (2 if kind == "reverse" else 1)) % 3] = 0.9
    lt = np.log(P) - 5.0
    if kind == "no_diagonal":
        lt[np.arange(3), np.arange(3)] = NINF
    return lt


def assert_equals_one_shot(s, want):
    """the closed session `s` (restatement) against a result of `segment_trans_logs`"""
    assert s.join_failures == 0
    assert s.F == len(want["cls"]) == s.p
    assert s.cls == want["cls"].tolist() and s.state == want["state"].tolist() and s.entered == want["entered"].tolist()
    assert np.array_equal(_bits(s.exit_score), _bits(want["exit_score"]))
    assert _bits(s.log_prob) == _bits(want["log_prob"]) and s.status == want["status"]


# ---- the streaming restatement == the one-shot restatement on the concatenation ------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "sparse"])
@pytest.mark.parametrize("Ns", [(5,) * 13, (3, 64, 7, 7, 33), (1, 1, 2)], ids=["5x13", "mixed", "tiny"])
def test_stream_restatement_equals_the_one_shot_restatement(kind, Ns):
    M, T, K = 8, 300, len(Ns)
    models = random_models(Ns, M, 21, 0.5 if kind == "sparse" else 0.0)
    lms = [V.log_model(*m) for m in models]
    rng = np.random.default_rng(K)
    seq = rng.integers(0, M, T)
    lt = cases.random_prices(rng, K, 0.2)
    want = RT.segment_trans_logs(lms, seq, lt)
    assert want["status"] == 0  # (the equality is claimed for such a stream; an input that dies would be replaced)
    cls, state, entered, ex, lp, st = RT.transcribe(models, seq, lt)
    assert (want["cls"].tolist(), want["state"].tolist(), want["entered"].tolist()) == (cls, state, entered)
    assert np.array_equal(_bits(want["exit_score"]), _bits(ex)) and _bits(want["log_prob"]) == _bits(lp) and st == 0
    for B in (1, 63, 64, 65, 100):
        counts = None
        for name, feeds in feed_patterns(T, B).items():
            s, finals = ST.decode(lms, seq, lt, B, feeds)
            assert_equals_one_shot(s, want)
            # the number of final frames is a function of the processed symbols alone, whatever the feeds were
            at = 0
            for n, fin in zip(feeds, finals):
                at += n
                assert fin == s.final_after(at // B * B), (B, name, at)
            by_p = [s.final_after(p) for p in range(0, T + 1, B)]
            assert counts is None or counts == by_p
            counts = by_p
            assert all(a <= b for a, b in zip(by_p, by_p[1:]))  # (monotone in p)


def test_flush_and_status_rules_of_the_restatement():
    M, B = 8, 16
    lms = [V.log_model(*m) for m in random_models((3, 4), M, 2)]
    lt = np.array([[-1.0, -2.0], [-0.5, -3.0]])
    seq = np.random.default_rng(0).integers(0, M, 200)
    want = RT.segment_trans_logs(lms, seq, lt)
    s = ST.Stream(lms, lt, 64)
    s.feed(seq[:70])
    assert (s.p, len(s.buf)) == (64, 6)
    s.flush()
    assert (s.p, len(s.buf)) == (70, 0) and s.F == s.final_after(70)
    s.feed(seq[70:])  # blocks now start at frame 70
    assert (s.p, len(s.buf)) == (70 + 128, 2)
    s.close()
    assert_equals_one_shot(s, want)
    # nothing fed
    s = ST.Stream(lms, lt, B)
    s.feed([])
    s.close()
    assert (s.F, s.log_prob, s.status) == (0, 0.0, 0)
    # a symbol >= M in the third block: the feed fails naming the frame, nothing of that feed is decided, close fills the rest
    seq = np.random.default_rng(0).integers(0, M, 60)
    seq[37] = M
    s = ST.Stream(lms, lt, B)
    s.feed(seq[:32])
    F0, head = s.F, (list(s.cls), list(s.exit_score))
    assert F0 > 0
    with pytest.raises(ST.BadSymbol) as ei:
        s.feed(seq[32:])
    assert ei.value.frame == 37 and s.F == F0
    out = s.close()
    assert (s.status, s.log_prob, s.F) == (2, NINF, 60)
    assert (s.cls[:F0], s.exit_score[:F0]) == head
    assert out["first"] == F0 and out["cls"] == [0xFFFF] * (60 - F0) and out["entered"] == [0] * (60 - F0)
    assert out["exit_score"] == [NINF] * (60 - F0)
    # ... in the first block: frame 0 was not final, and is filled as the closed decode fills it
    seq[5] = M
    s = ST.Stream(lms, lt, B)
    with pytest.raises(ST.BadSymbol):
        s.feed(seq)
    out = s.close()
    closed = RT.segment_trans_logs(lms, seq, lt)
    assert closed["status"] == 2 and out["cls"] == closed["cls"].tolist() and out["entered"] == closed["entered"].tolist()
    assert np.array_equal(_bits(out["exit_score"]), _bits(closed["exit_score"])) and out["exit_score"][0] == 0.0


@pytest.mark.parametrize("case", [c[0] for c in cases.uniform_cases()])
def test_one_price_everywhere_the_two_one_shot_restatements_agree_on_the_path(case):
    """the inputs on which the GPU test holds the matrix session against hmm.SegmentStream"""
    _name, models, streams = next(c for c in cases.uniform_cases() if c[0] == case)
    K = len(models)
    lms = [V.log_model(*m) for m in models]
    for seq in streams:
        u = RT.segment_trans_logs(lms, seq, np.full((K, K), cases.UNIFORM_PRICE))
        r = R1.segment_logs(lms, seq, cases.UNIFORM_PRICE)
        assert u["cls"].tolist() == r["cls"].tolist() and u["state"].tolist() == r["state"].tolist()
        assert u["entered"].tolist() == r["entered"].tolist() and u["status"] == r["status"]
        assert _bits(u["log_prob"]) == _bits(r["log_prob"])


# ---- the planted stream: frames are decided long before the end ---------------------------------------------------------------
PLANTED_FINALS = [57, 62, 165, 249, 318, 374, 416]  # after the seven whole blocks of 64


@pytest.mark.parametrize("kind", ["cycle", "no_diagonal", "reverse"])
def test_on_the_planted_stream_half_of_the_processed_frames_are_final_from_the_third_block_on(kind):
    models = planted_models()
    sym = planted_stream(models, np.random.default_rng(3))
    assert len(sym) == 510
    lms = [V.log_model(*m) for m in models]
    lt = planted_prices(kind)
    B = 64
    s, finals = ST.decode(lms, sym, lt, B, [B] * (len(sym) // B) + [len(sym) % B])
    print(kind, "final after each block:", finals[:-1], "peak pending:", s.peak_pending)
    assert_equals_one_shot(s, RT.segment_trans_logs(lms, sym, lt))
    for i, fin in enumerate(finals[:len(sym) // B]):
        if i >= 2:  # (after the second block 62 of 128 are final: the one-price test's "from the second block on" does not hold)
            assert 2 * fin >= (i + 1) * B, (i, fin)
    assert s.peak_pending < 3 * B
    assert finals[:-1] == PLANTED_FINALS and s.peak_pending <= 130


def test_where_every_price_is_forbidden_nothing_is_final_before_close():
    models = planted_models()
    sym = planted_stream(models, np.random.default_rng(3))
    lms = [V.log_model(*m) for m in models]
    lt = np.full((3, 3), NINF)
    B = 64
    s, finals = ST.decode(lms, sym, lt, B, [B] * (len(sym) // B) + [len(sym) % B])
    assert finals == [0] * len(finals)
    assert_equals_one_shot(s, RT.segment_trans_logs(lms, sym, lt))
    # and under a budget of three blocks the fourth does not fit, while close still decides everything that was taken
    s = ST.Stream(lms, lt, B, cap=3 * B)
    s.feed(sym[:3 * B])
    with pytest.raises(ST.RingFull) as ei:
        s.feed(sym[3 * B:4 * B + 5])
    assert (ei.value.pending, ei.value.taken) == (3 * B, 0)
    s.close()
    assert_equals_one_shot(s, RT.segment_trans_logs(lms, sym[:3 * B], lt))


# ---- e2vq_hmm_segment_trans_stream_open: refusals before the device ------------------------------------------------------------
def _open_c(models, lt, Ns=None, K=None, M=8):
    Ns = [len(m[0]) for m in models] if Ns is None else Ns
    K = len(models) if K is None else K
    n = max(len(models), 1)
    ns = (C.c_int * n)(*Ns)
    keep = [[np.ascontiguousarray(m[i], dtype=np.float64) for m in models] for i in range(3)]
    ptr = lambda i: (C.c_void_p * n)(*[a.ctypes.data for a in keep[i]])
    lt = None if lt is None else np.ascontiguousarray(lt, dtype=np.float64)
    h = C.c_void_p()
    rc = e.lib.e2vq_hmm_segment_trans_stream_open(0, K, ns, M, ptr(0), ptr(1), ptr(2), None if lt is None else lt.ctypes.data, C.byref(h))
    assert rc == 0 or not h
    return rc, h


def _bad(where, value):
    pi, A, B = (x.copy() for x in _uniform(3, 8))
    {"pi": pi, "A": A, "B": B}[where].flat[1] = value
    return pi, A, B


@pytest.mark.parametrize("case,needle", [
    ("K0", "e2vq_hmm_segment_trans_stream_open: 0 models (at least 1)"),
    ("N0", "e2vq_hmm_segment_trans_stream_open: model 1 has N=0 states (1 .. 64)"),
    ("N65", "e2vq_hmm_segment_trans_stream_open: model 0 has N=65 states (1 .. 64)"),
    ("sumN", "e2vq_hmm_segment_trans_stream_open: 4160 states in all models (at most 4096)"),
    ("no_lt", "e2vq_hmm_segment_trans_stream_open: bad arguments"),
    ("lt_nan", "e2vq_hmm_segment_trans_stream_open: lt[1][0] = nan: the logarithm of a price, at most 0 (-inf forbids the succession)"),
    ("lt_pos", "e2vq_hmm_segment_trans_stream_open: lt[0][1] = 0.5: the logarithm of a price, at most 0 (-inf forbids the succession)"),
    ("negative", "HMM parameter A[1] = -0.25: not a finite non-negative number"),
    ("nan", "HMM parameter pi[1] = nan: not a finite non-negative number"),
    ("slots", "e2vq_hmm_segment_trans_stream_open: the classes take 17 wave-slots of 64 lanes (at most 16"),
    ("block_0", "e2vq_hmm_segment_trans_stream_open: ECOZ2_HMM_SEGMENT_STREAM_BLOCK=0: a block of 1 .."),
    ("block_word", "e2vq_hmm_segment_trans_stream_open: ECOZ2_HMM_SEGMENT_STREAM_BLOCK=many: a block of 1 .."),
    ("budget", "ECOZ2_HMM_SEGMENT_STREAM_PENDING_BYTES=4607 holds 127 pending frames of 6 states and 2 classes (36 bytes a frame): "
               "fewer than two blocks of 64"),
])
def test_open_refuses_before_the_device(case, needle, monkeypatch):
    ok = _uniform(3, 8)
    kw, models = {}, [ok, ok]
    lt = np.array([[-1.0, -2.0], [NINF, 0.0]])
    if case == "K0":
        kw["K"] = 0
    elif case == "N0":
        kw["Ns"] = [3, 0]
    elif case == "N65":
        models, lt = [_uniform(65, 8)], np.zeros((1, 1))
    elif case == "sumN":
        models, lt = [_uniform(64, 8)] * 65, np.zeros((65, 65))
    elif case == "no_lt":
        lt = None
    elif case == "lt_nan":
        lt[1, 0] = float("nan")
    elif case == "lt_pos":
        lt[0, 1] = 0.5
    elif case == "negative":
        models = [ok, _bad("A", -0.25)]
    elif case == "nan":
        models = [_bad("pi", float("nan")), ok]
    elif case == "slots":
        models, lt = [_uniform(64, 8)] * 17, np.zeros((17, 17))
    elif case.startswith("block"):
        monkeypatch.setenv(ENV_BLOCK, {"block_0": "0", "block_word": "many"}[case])
    else:
        monkeypatch.setenv(ENV_BLOCK, "64")
        monkeypatch.setenv(ENV_PENDING, str(2 * 64 * 36 - 1))
    rc, _h = _open_c(models, lt, **kw)
    assert rc == 1 and needle in _err(), _err()


def test_python_mirror_raises_the_refusal():
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.SegmentTransStream([_uniform(3, 8)], [[1.0]])
    assert "lt[0][0] = 1" in str(ei.value)
    with pytest.raises(ValueError):
        hmm.SegmentTransStream([_uniform(3, 8)], np.zeros((2, 2)))
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.SegmentTransStream([_uniform(64, 8)] * 17, np.zeros((17, 17)))
    assert "the classes take 17 wave-slots" in str(ei.value)
    with pytest.raises(ValueError):
        hmm.segment_files(["a.hmm"], ["x.seq"], -1.0, grammar_continuous="rec")  # (no class_transitions)
    for kw in (dict(continuous="r"), dict(posteriors=True), dict(grammar_posteriors=True), dict(frame_posteriors="d"), dict(body="looped")):
        with pytest.raises(ValueError):
            hmm.segment_files(["a.hmm"], ["x.seq"], -1.0, class_transitions="t.csv", grammar_continuous="rec", **kw)
    with pytest.raises(ValueError):  # (as before this mode existed)
        hmm.segment_files(["a.hmm"], ["x.seq"], -1.0, class_transitions="t.csv", continuous="rec")


# ---- e2vq_hmm_segment_trans_continuous_files and the CLI: refusals ------------------------------------------------------------
@pytest.fixture
def corpus(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    models = []
    for c, N in (("A", 3), ("B", 5)):
        hmm.save_model(d / f"{c}.hmm", c, *_uniform(N, 16))
        models.append(str(d / f"{c}.hmm"))
    hmm.save_model(d / "A2.hmm", "A", *_uniform(4, 16))
    hmm.save_model(d / "N65.hmm", "D", *_uniform(65, 16))
    (d / "many").mkdir()
    for k in range(17):
        hmm.save_model(d / "many" / f"c{k:02d}.hmm", f"c{k:02d}", *_uniform(64, 16))
    e.formats.write_seq(str(d / "x.seq"), "A", 16, np.arange(40) % 16)
    e.formats.write_seq(str(d / "y32.seq"), "A", 32, np.arange(40) % 32)
    e.formats.write_prd(str(d / "x.prd"), "A", np.random.default_rng(1).uniform(0.1, 1.0, (40, 5)))
    (d / "t.csv").write_text("class,A,B\nA,0,-1\nB,-2,-inf\n")
    (d / "t3.csv").write_text("class,A,B,C\nA,0,-1,0\nB,-2,-inf,0\nC,0,0,0\n")
    (d / "tpos.csv").write_text("class,A,B\nA,0,-1\nB,2,-inf\n")
    (d / "notes.txt").write_text("x")
    return tmp_path, d, models


def _files(models, inputs, out, transitions, name=b"rec", ls=-5.0):
    m, _k1 = hmm._strs(models)
    f, _k2 = hmm._strs(inputs)
    return e.lib.e2vq_hmm_segment_trans_continuous_files(m, len(models), None, f, len(inputs), 4, 45, 15, ls,
                                                         str(transitions).encode() if transitions else None, name, str(out).encode())


@pytest.mark.parametrize("case,needle", [
    ("no_models", "e2vq_hmm_segment_trans_continuous_files: no models"),
    ("no_inputs", "e2vq_hmm_segment_trans_continuous_files: no inputs"),
    ("no_name", "e2vq_hmm_segment_trans_continuous_files: the recording needs a name"),
    ("no_file", "e2vq_hmm_segment_trans_continuous_files: no class-transitions file"),
    ("switch_pos", "e2vq_hmm_segment_trans_continuous_files: ln_switch = 2"),
    ("N65", "e2vq_hmm_segment_trans_continuous_files: model 2 has N=65 states (1 .. 64)"),
    ("slots", "e2vq_hmm_segment_trans_continuous_files: the classes take 17 wave-slots of 64 lanes (at most 16"),
    ("same_class", "e2vq_hmm_segment_trans_continuous_files: two models of the class 'A'"),
    ("missing", "none.csv"),
    ("names", "t3.csv:1: 3 class names for 2 models"),
    ("value", "tpos.csv:3: B -> A = 2: the logarithm of a price"),
    ("seq_M", "y32.seq: codebook size 32 differs from the models' 16"),
    ("no_codebook", "e2vq_hmm_segment_trans_continuous_files: signals and predictors need a codebook"),
    ("extension", "notes.txt: not a .wav, .prd or .seq file"),
    ("block", "ECOZ2_HMM_SEGMENT_STREAM_BLOCK=0: a block of 1 .."),
])
def test_trans_continuous_files_refuses_before_the_device(corpus, case, needle, monkeypatch):
    tmp_path, d, models = corpus
    inputs, transitions, kw = [str(d / "x.seq"), str(d / "x.seq")], d / "t.csv", {}
    if case == "no_models":
        models = []
    elif case == "no_inputs":
        inputs = []
    elif case == "no_name":
        kw["name"] = b""
    elif case == "no_file":
        transitions = None
    elif case == "switch_pos":
        kw["ls"] = 2.0
    elif case == "N65":
        models = models + [str(d / "N65.hmm")]
    elif case == "slots":
        models = [str(d / "many" / f"c{k:02d}.hmm") for k in range(17)]
    elif case == "same_class":
        models = models + [str(d / "A2.hmm")]
    elif case == "missing":
        transitions = d / "none.csv"
    elif case == "names":
        transitions = d / "t3.csv"
    elif case == "value":
        transitions = d / "tpos.csv"
    elif case == "seq_M":
        inputs = [str(d / "x.seq"), str(d / "y32.seq")]
    elif case == "no_codebook":
        inputs = [str(d / "x.prd")]
    elif case == "extension":
        inputs = [str(d / "notes.txt")]
    else:
        monkeypatch.setenv(ENV_BLOCK, "0")
    out = tmp_path / "out"
    assert _files(models, inputs, out, transitions, **kw) == 1
    assert needle in _err(), _err()
    assert not out.exists()


def _cli(cwd, *args):
    r = subprocess.run([EXE, "hmm", "segment", *args], cwd=cwd, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


OWN = "hmm segment: --grammar-continuous decodes one stream under the prices of --class-transitions: not with --continuous, " \
      "--posteriors, --grammar-posteriors, --frame-posteriors or --body"


@pytest.mark.parametrize("args,code,needle", [
    (["--grammar-continuous", "rec"], 2, "hmm segment: --grammar-continuous needs --class-transitions <file.csv>"),
    (["--grammar-continuous", "rec", "--class-transitions", "in/t.csv", "--continuous", "rec"], 2, OWN),
    (["--grammar-continuous", "rec", "--class-transitions", "in/t.csv", "--posteriors"], 2, OWN),
    (["--grammar-continuous", "rec", "--class-transitions", "in/t.csv", "--grammar-posteriors"], 2, OWN),
    (["--grammar-continuous", "rec", "--class-transitions", "in/t.csv", "--frame-posteriors", "fp"], 2, OWN),
    (["--grammar-continuous", "rec", "--class-transitions", "in/t.csv", "--body", "looped"], 2, OWN),
    (["--grammar-continuous"], 2, "--grammar-continuous needs a value"),
    (["--grammar-continuous", "", "--class-transitions", "in/t.csv"], 2, "hmm segment: --grammar-continuous <name>: the recording needs a name"),
    (["--grammar-continuous", "rec", "--class-transitions", "in/t.csv", "--models", "in/N65.hmm"], 1, "model 1 has N=65 states (1 .. 64)"),
    # the pair the one-price mode refuses keeps its message
    (["--continuous", "rec", "--class-transitions", "in/t.csv"], 2,
     "hmm segment: --continuous decodes under the one switch penalty: not with --posteriors or --class-transitions"),
])
def test_cli_refusals(corpus, args, code, needle):
    tmp_path, _d, _models = corpus
    rc, out, err = _cli(tmp_path, "--models", "in/A.hmm", "--sequences", "in/x.seq", "--switch-penalty", "-5", "-c", "out", *args)
    assert rc == code and needle in (err if code == 2 else out), (rc, out, err)
    assert not (tmp_path / "out").exists() and not (tmp_path / "fp").exists()


def test_usage_has_a_line_of_its_own_beneath_the_old_ones(tmp_path):
    rc, _out, err = _cli(tmp_path)
    assert rc == 2
    new = ("  ecoz2 hmm segment -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15]\n"
           "                  --switch-penalty <x <= 0 | -inf> --class-transitions <file.csv> --grammar-continuous <name>\n")
    assert new in err
    assert "(--grammar-continuous <name>: the inputs are consecutive pieces of one recording, decoded as one stream\n" in err
    old = ("  ecoz2 hmm segment -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15]\n"
           "                  --switch-penalty <x <= 0 | -inf> [-c <csv dir|file.csv>]\n"
           "                  [--posteriors [--frame-posteriors <dir>]]\n"
           "                  [--body <auto|resident|looped>]\n"
           "                  [--class-transitions <file.csv>]\n"
           "                  [--grammar-posteriors [--frame-posteriors <dir>]]\n"
           "                  [--continuous <name>]\n")
    assert old in err and err.index(old) < err.index(new)
    assert "                  (--continuous <name>: the inputs are consecutive pieces of one recording, decoded as one stream)\n" in err
    assert err.index("(--continuous <name>:") < err.index(new) < err.index("  ecoz2 hmm transitions -m|--models")


def test_library_exports():
    for name in ("e2vq_hmm_segment_trans_stream_open", "e2vq_hmm_segment_trans_continuous_files"):
        assert hasattr(e.lib, name)
    assert issubclass(hmm.SegmentTransStream, hmm.SegmentStream)
    for name in ("feed", "flush", "close", "take", "kernel_ms", "stats", "__enter__", "__exit__"):
        assert callable(getattr(hmm.SegmentTransStream, name))
    assert isinstance(hmm.SegmentTransStream.final_frames, property)
    import inspect
    assert "grammar_continuous" in inspect.signature(hmm.segment_files).parameters


# ---- compiler metadata (read as test_hmm_segment_stream_cpu.py reads its kernels') -----------------------------------------------
VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_segment_trans_stream.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_segment_trans_stream.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _meta(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    return lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))


@pytest.mark.parametrize("pattern", [r"k_hmm_segment_trans_streamILb0ELb0E", r"k_hmm_segment_trans_streamILb0ELb1E",
                                     r"k_hmm_segment_trans_streamILb1ELb0E", r"k_hmm_segment_trans_streamILb1ELb1E",
                                     r"k_hmm_segment_trans_coalesceE", r"k_hmm_segment_trans_stream_backtrackE"])
def test_trans_stream_kernels_have_no_scratch_no_spill_and_fit_their_budget(asm, pattern):
    g = _meta(asm, pattern)
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
