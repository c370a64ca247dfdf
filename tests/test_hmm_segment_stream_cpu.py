"""`hmm segment --continuous`, CPU side: the streaming restatement against `segment_logs` / `transcribe` on
the concatenation for every block length and feed pattern; on a planted stream, that frames are decided long before the end
(and never without switching); the refusals of the session, of e2vq_hmm_segment_continuous_files and of the CLI, which come
before any HIP call; the exports and the usage text; the kernels' compiler metadata.  The GPU tests are in
test_gpu_hmm_segment_stream.py (a session cannot be opened without a device, so "feed after close" is there)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_segment_restatement as R
from . import hmm_segment_stream_restatement as S
from . import hmm_viterbi_restatement as V

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


def random_models(Ns, M, seed, zeros=0.0):
    """rows drawn at random; `zeros`: the share of entries of pi and A set to 0 (a row keeps at least one entry)"""
    rng = np.random.default_rng(seed)

    def rows(n, m, z):
        x = rng.uniform(0.05, 1.0, (n, m))
        if z:
            x[rng.uniform(size=(n, m)) < z] = 0.0
            x[np.arange(n), rng.integers(0, m, n)] += 0.5
        return x / x.sum(axis=1, keepdims=True)
    return [(rows(1, N, zeros)[0], rows(N, N, zeros), rows(N, M, 0.0)) for N in Ns]


def feed_patterns(T, seed):
    """all at once; one symbol at a time; random lengths, empty feeds among them"""
    rng = np.random.default_rng(seed)
    rand = []
    while sum(rand) < T:
        rand.append(int(min(rng.choice([0, 0, 1, 5, 17, 64, 90, 130]), T - sum(rand))))
    return {"whole": [T], "single": [1] * T, "random": rand + [0]}


def assert_equals_one_shot(s, want):
    """the closed session `s` (restatement) against a result of `segment_logs`"""
    assert s.join_failures == 0
    assert s.F == len(want["cls"]) == s.p
    assert s.cls == want["cls"].tolist() and s.state == want["state"].tolist() and s.entered == want["entered"].tolist()
    assert np.array_equal(_bits(s.gbest), _bits(want["gbest"]))
    assert _bits(s.log_prob) == _bits(want["log_prob"]) and s.status == want["status"]


# ---- the streaming restatement == the one-shot restatement on the concatenation ------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "sparse"])
@pytest.mark.parametrize("Ns", [(5,) * 13, (3, 64, 7, 7, 33), (1, 1, 2)], ids=["5x13", "mixed", "tiny"])
def test_stream_restatement_equals_the_one_shot_restatement(kind, Ns):
    M, T, ls = 8, 300, -2.0
    models = random_models(Ns, M, 21, 0.5 if kind == "sparse" else 0.0)
    lms = [V.log_model(*m) for m in models]
    seq = np.random.default_rng(len(Ns)).integers(0, M, T)
    want = R.segment_logs(lms, seq, ls)
    assert want["status"] == 0
    cls, state, entered, G, lp, st = R.transcribe(models, seq, ls)
    assert (want["cls"].tolist(), want["state"].tolist(), want["entered"].tolist()) == (cls, state, entered)
    assert np.array_equal(_bits(want["gbest"]), _bits(G)) and _bits(want["log_prob"]) == _bits(lp) and st == 0
    for B in (1, 63, 64, 65, 100):
        counts = None
        for name, feeds in feed_patterns(T, B).items():
            s, finals = S.decode(lms, seq, ls, B, feeds)
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


def test_flush_processes_the_remainder_and_the_next_block_starts_there():
    M, T, ls, B = 8, 200, -2.0, 64
    lms = [V.log_model(*m) for m in random_models((3, 4), M, 2)]
    seq = np.random.default_rng(0).integers(0, M, T)
    want = R.segment_logs(lms, seq, ls)
    s = S.Stream(lms, ls, B)
    s.feed(seq[:70])
    assert (s.p, len(s.buf)) == (64, 6)
    s.flush()
    assert (s.p, len(s.buf)) == (70, 0) and s.F == s.final_after(70)
    s.feed(seq[70:])  # blocks now start at frame 70
    assert (s.p, len(s.buf)) == (70 + 128, 2)
    s.close()
    assert_equals_one_shot(s, want)


def test_empty_stream_and_status_rules_of_the_restatement():
    M, ls, B = 8, -2.0, 16
    lms = [V.log_model(*m) for m in random_models((3, 4), M, 2)]
    s = S.Stream(lms, ls, B)
    s.feed([])
    s.close()
    assert (s.F, s.log_prob, s.status) == (0, 0.0, 0)
    # a symbol >= M in the third block: the feed fails naming the frame, nothing of that feed is decided, close fills the rest
    seq = np.random.default_rng(0).integers(0, M, 60)
    seq[37] = M
    s = S.Stream(lms, ls, B)
    s.feed(seq[:32])
    F0, head = s.F, (list(s.cls), list(s.gbest))
    with pytest.raises(S.BadSymbol) as ei:
        s.feed(seq[32:])
    assert ei.value.frame == 37 and s.F == F0
    out = s.close()
    assert (s.status, s.log_prob, s.F) == (2, NINF, 60)
    assert (s.cls[:F0], s.gbest[:F0]) == head
    assert out["first"] == F0 and out["cls"] == [0xFFFF] * (60 - F0) and out["entered"] == [0] * (60 - F0) and out["gbest"] == [NINF] * (60 - F0)


# ---- a planted stream: frames are decided long before the end ---------------------------------------------------------------------
PLANTED = [(0, 120), (2, 80), (1, 150), (0, 60), (2, 100)]


def planted_models():
    """three classes, N = 4, M = 16: B peaked on disjoint symbol groups (class k on symbols 5 k .. 5 k + 4, 70 % of the
    mass, each state leaning to one symbol of the group), A diagonal-heavy, pi uniform"""
    N, M = 4, 16
    models = []
    for k in range(3):
        B = np.full((N, M), 0.3 / (M - 5))
        for j in range(N):
            w = np.full(5, 1.0)
            w[j] = 3.0
            B[j, 5 * k:5 * k + 5] = 0.7 * w / w.sum()
        A = np.full((N, N), 0.1 / (N - 1))
        A[np.arange(N), np.arange(N)] = 0.9
        models.append((np.full(N, 1.0 / N), A, B))
    return models


def planted_stream(models, rng):
    sym = []
    for k, n in PLANTED:
        pi, A, B = models[k]
        j = rng.choice(len(pi), p=pi)
        for _ in range(n):
            sym.append(rng.choice(B.shape[1], p=B[j]))
            j = rng.choice(len(pi), p=A[j])
    return np.array(sym, dtype=np.uint16)


def test_on_the_planted_stream_half_of_the_processed_frames_are_final_from_the_second_block_on():
    models = planted_models()
    sym = planted_stream(models, np.random.default_rng(3))
    lms = [V.log_model(*m) for m in models]
    B = 64
    s, finals = S.decode(lms, sym, -5.0, B, [B] * (len(sym) // B) + [len(sym) % B])
    print("final after each block:", finals[:-1], "peak pending:", s.peak_pending)
    assert_equals_one_shot(s, R.segment_logs(lms, sym, -5.0))
    for i, fin in enumerate(finals[:len(sym) // B]):
        if i >= 1:
            assert 2 * fin >= (i + 1) * B, (i, fin)
    assert s.peak_pending < 2 * B


def test_without_switching_nothing_is_final_before_close():
    models = planted_models()
    sym = planted_stream(models, np.random.default_rng(3))
    lms = [V.log_model(*m) for m in models]
    B = 64
    s, finals = S.decode(lms, sym, NINF, B, [B] * (len(sym) // B) + [len(sym) % B])
    assert finals == [0] * len(finals)
    assert_equals_one_shot(s, R.segment_logs(lms, sym, NINF))
    # and under a budget of three blocks the fourth does not fit, while close still decides everything that was taken
    s = S.Stream(lms, NINF, B, cap=3 * B)
    s.feed(sym[:3 * B])
    with pytest.raises(S.RingFull) as ei:
        s.feed(sym[3 * B:4 * B + 5])
    assert (ei.value.pending, ei.value.taken) == (3 * B, 0)
    s.close()
    assert_equals_one_shot(s, R.segment_logs(lms, sym[:3 * B], NINF))


# ---- e2vq_hmm_segment_stream_*: refusals before the device -------------------------------------------------------------------------
def _open_c(models, ln_switch, Ns=None, K=None, M=8):
    Ns = [len(m[0]) for m in models] if Ns is None else Ns
    K = len(models) if K is None else K
    n = max(len(models), 1)
    ns = (C.c_int * n)(*Ns)
    keep = [[np.ascontiguousarray(m[i], dtype=np.float64) for m in models] for i in range(3)]
    ptr = lambda i: (C.c_void_p * n)(*[a.ctypes.data for a in keep[i]])
    h = C.c_void_p()
    rc = e.lib.e2vq_hmm_segment_stream_open(0, K, ns, M, ptr(0), ptr(1), ptr(2), ln_switch, C.byref(h))
    assert rc == 0 or not h
    return rc, h


def _bad(where, value):
    pi, A, B = (x.copy() for x in _uniform(3, 8))
    {"pi": pi, "A": A, "B": B}[where].flat[1] = value
    return pi, A, B


@pytest.mark.parametrize("case,needle", [
    ("K0", "e2vq_hmm_segment_stream_open: 0 models (at least 1)"),
    ("N0", "e2vq_hmm_segment_stream_open: model 1 has N=0 states (1 .. 64)"),
    ("N65", "e2vq_hmm_segment_stream_open: model 0 has N=65 states (1 .. 64)"),
    ("sumN", "e2vq_hmm_segment_stream_open: 4160 states in all models (at most 4096)"),
    ("negative", "HMM parameter A[1] = -0.25: not a finite non-negative number"),
    ("nan", "HMM parameter pi[1] = nan: not a finite non-negative number"),
    ("inf", "HMM parameter B[1] = inf: not a finite non-negative number"),
    ("switch_nan", "e2vq_hmm_segment_stream_open: ln_switch = nan"),
    ("switch_pos", "e2vq_hmm_segment_stream_open: ln_switch = 0.5"),
    ("block_0", "e2vq_hmm_segment_stream_open: ECOZ2_HMM_SEGMENT_STREAM_BLOCK=0: a block of 1 .."),
    ("block_neg", "e2vq_hmm_segment_stream_open: ECOZ2_HMM_SEGMENT_STREAM_BLOCK=-4: a block of 1 .."),
    ("block_word", "e2vq_hmm_segment_stream_open: ECOZ2_HMM_SEGMENT_STREAM_BLOCK=many: a block of 1 .."),
    ("budget", "ECOZ2_HMM_SEGMENT_STREAM_PENDING_BYTES=1279 holds 127 pending frames of 3 states (10 bytes a frame): fewer than two "
               "blocks of 64"),
    ("body", "ECOZ2_HMM_SEGMENT_BODY=fast: resident or looped"),
])
def test_open_refuses_before_the_device(case, needle, monkeypatch):
    ok = _uniform(3, 8)
    ls, kw, models = -1.0, {}, [ok]
    if case == "K0":
        kw["K"] = 0
    elif case == "N0":
        models, kw["Ns"] = [ok, ok], [3, 0]
    elif case == "N65":
        models = [_uniform(65, 8)]
    elif case == "sumN":
        models = [_uniform(64, 8)] * 65
    elif case == "negative":
        models = [ok, _bad("A", -0.25)]
    elif case == "nan":
        models = [_bad("pi", float("nan"))]
    elif case == "inf":
        models = [_bad("B", float("inf"))]
    elif case == "switch_nan":
        ls = float("nan")
    elif case == "switch_pos":
        ls = 0.5
    elif case.startswith("block"):
        monkeypatch.setenv(ENV_BLOCK, {"block_0": "0", "block_neg": "-4", "block_word": "many"}[case])
    elif case == "budget":
        monkeypatch.setenv(ENV_BLOCK, "64")
        monkeypatch.setenv(ENV_PENDING, str(2 * 64 * 10 - 1))
    else:
        monkeypatch.setenv("ECOZ2_HMM_SEGMENT_BODY", "fast")
    rc, _h = _open_c(models, ls, **kw)
    assert rc == 1 and needle in _err(), _err()


def test_a_null_session_is_refused():
    fin = C.c_int64()
    sym = np.zeros(4, np.uint16)
    assert e.lib.e2vq_hmm_segment_stream_feed(None, sym.ctypes.data, 4, 0, C.byref(fin)) == 1
    assert "e2vq_hmm_segment_stream_feed: NULL session" in _err()
    assert e.lib.e2vq_hmm_segment_stream_flush(None, C.byref(fin)) == 1 and "e2vq_hmm_segment_stream_flush: NULL session" in _err()
    assert e.lib.e2vq_hmm_segment_stream_close(None, None, None, None) == 1 and "e2vq_hmm_segment_stream_close: NULL session" in _err()
    assert e.lib.e2vq_hmm_segment_stream_take(None, 1, None, None, None, None, None, None) == 1
    assert "e2vq_hmm_segment_stream_take: NULL session" in _err()
    ms = C.c_float()
    assert e.lib.e2vq_hmm_segment_stream_kernel_ms(None, C.byref(ms)) == 1 and "NULL session" in _err()
    e.lib.e2vq_hmm_segment_stream_free(None)


def test_python_mirror_raises_the_refusal():
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.SegmentStream([_uniform(3, 8)], 1.0)
    assert "ln_switch = 1" in str(ei.value)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.SegmentStream([], -1.0)
    assert "0 models (at least 1)" in str(ei.value)
    with pytest.raises(ValueError):
        hmm.segment_files(["a.hmm"], ["x.seq"], -1.0, posteriors=True, continuous="rec")


# ---- e2vq_hmm_segment_continuous_files and the CLI: refusals ---------------------------------------------------------------------
@pytest.fixture
def corpus(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    models = []
    for c, N in (("A", 3), ("B", 5)):
        hmm.save_model(d / f"{c}.hmm", c, *_uniform(N, 16))
        models.append(str(d / f"{c}.hmm"))
    hmm.save_model(d / "C32.hmm", "C", *_uniform(3, 32))
    hmm.save_model(d / "N65.hmm", "D", *_uniform(65, 16))
    rng = np.random.default_rng(1)
    e.formats.write_cbook(str(d / "m16p6.cbook"), "_", rng.uniform(-0.5, 0.5, (16, 7)))
    e.formats.write_prd(str(d / "x.prd"), "A", rng.uniform(0.1, 1.0, (40, 5)))
    e.formats.write_seq(str(d / "x.seq"), "A", 16, np.arange(40) % 16)
    e.formats.write_seq(str(d / "y32.seq"), "A", 32, np.arange(40) % 32)
    (d / "notes.txt").write_text("x")
    return tmp_path, d, models


def _continuous_files(models, inputs, out, name=b"rec", codebook=None, ls=-5.0):
    m, _k1 = hmm._strs(models)
    f, _k2 = hmm._strs(inputs)
    return e.lib.e2vq_hmm_segment_continuous_files(m, len(models), str(codebook).encode() if codebook else None, f, len(inputs), 4, 45,
                                                   15, ls, name, str(out).encode())


@pytest.mark.parametrize("case,needle", [
    ("no_models", "e2vq_hmm_segment_continuous_files: no models"),
    ("no_inputs", "e2vq_hmm_segment_continuous_files: no inputs"),
    ("no_name", "e2vq_hmm_segment_continuous_files: the recording needs a name"),
    ("switch_pos", "e2vq_hmm_segment_continuous_files: ln_switch = 2"),
    ("N65", "e2vq_hmm_segment_continuous_files: model 2 has N=65 states (1 .. 64)"),
    ("models_M", "model has M=32 but"),
    ("cb_P_prd", "x.prd: prediction order 4 differs from the codebook's 6"),
    ("seq_M", "y32.seq: codebook size 32 differs from the models' 16"),
    ("no_codebook", "e2vq_hmm_segment_continuous_files: signals and predictors need a codebook"),
    ("extension", "notes.txt: not a .wav, .prd or .seq file"),
    ("block", "ECOZ2_HMM_SEGMENT_STREAM_BLOCK=0: a block of 1 .."),
])
def test_continuous_files_refuses_before_the_device(corpus, case, needle, monkeypatch):
    tmp_path, d, models = corpus
    kw = {}
    inputs = [str(d / "x.seq"), str(d / "x.seq")]
    if case == "no_models":
        models = []
    elif case == "no_inputs":
        inputs = []
    elif case == "no_name":
        kw["name"] = b""
    elif case == "switch_pos":
        kw["ls"] = 2.0
    elif case == "N65":
        models = models + [str(d / "N65.hmm")]
    elif case == "models_M":
        models = models + [str(d / "C32.hmm")]
    elif case == "cb_P_prd":
        kw["codebook"] = d / "m16p6.cbook"
        inputs = [str(d / "x.prd")]
    elif case == "seq_M":
        inputs = [str(d / "x.seq"), str(d / "y32.seq")]
    elif case == "no_codebook":
        inputs = [str(d / "x.prd")]
    elif case == "extension":
        inputs = [str(d / "notes.txt")]
    else:
        monkeypatch.setenv(ENV_BLOCK, "0")
    out = tmp_path / "out"
    assert _continuous_files(models, inputs, out, **kw) == 1
    assert needle in _err(), _err()
    assert not out.exists()


def _cli(cwd, *args):
    r = subprocess.run([EXE, "hmm", "segment", *args], cwd=cwd, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("args,code,needle", [
    (["--continuous", "rec", "--posteriors"], 2, "hmm segment: --continuous decodes under the one switch penalty: not with --posteriors"),
    (["--continuous", "rec", "--class-transitions", "in/t.csv"], 2, "not with --posteriors or --class-transitions"),
    (["--continuous"], 2, "--continuous needs a value"),
    (["--continuous", ""], 2, "hmm segment: --continuous <name>: the recording needs a name"),
    (["--continuous", "rec", "--models", "in/N65.hmm"], 1, "model 1 has N=65 states (1 .. 64)"),
])
def test_cli_refusals(corpus, args, code, needle):
    tmp_path, _d, _models = corpus
    rc, out, err = _cli(tmp_path, "--models", "in/A.hmm", "--sequences", "in/x.seq", "--switch-penalty", "-5", "-c", "out", *args)
    assert rc == code and needle in (err if code == 2 else out), (rc, out, err)
    assert not (tmp_path / "out").exists()


def test_usage_names_continuous_and_keeps_the_old_lines(tmp_path):
    rc, _out, err = _cli(tmp_path)
    assert rc == 2
    assert "                  [--continuous <name>]\n" in err
    assert "(--continuous <name>: the inputs are consecutive pieces of one recording, decoded as one stream)" in err
    assert "ecoz2 hmm segment -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15]" in err
    assert "--switch-penalty <x <= 0 | -inf> [-c <csv dir|file.csv>]" in err
    assert "[--posteriors [--frame-posteriors <dir>]]" in err and "[--class-transitions <file.csv>]" in err


def test_stream_library_exports():
    for name in ("open", "feed", "flush", "close", "take", "kernel_ms", "stats", "free"):
        assert hasattr(e.lib, "e2vq_hmm_segment_stream_" + name)
    assert hasattr(e.lib, "e2vq_hmm_segment_continuous_files")
    assert isinstance(hmm.SegmentStream.final_frames, property) and callable(hmm.SegmentStream.kernel_ms)
    for name in ("feed", "flush", "close", "__enter__", "__exit__"):
        assert callable(getattr(hmm.SegmentStream, name))


# ---- compiler metadata (read as test_hmm_segment_cpu.py reads its kernels') ---------------------------------------------------------
VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_segment_stream.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_segment_stream.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _meta(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    return lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))


@pytest.mark.parametrize("pattern", [r"k_hmm_segment_streamILb0ELb0E", r"k_hmm_segment_streamILb0ELb1E", r"k_hmm_segment_streamILb1ELb0E",
                                     r"k_hmm_segment_streamILb1ELb1E", r"k_hmm_segment_coalesceE", r"k_hmm_segment_stream_backtrackE"])
def test_stream_kernels_have_no_scratch_no_spill_and_fit_their_budget(asm, pattern):
    g = _meta(asm, pattern)
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
