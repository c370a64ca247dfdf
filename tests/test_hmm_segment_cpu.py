"""`hmm segment`, CPU side: the numpy restatement against the contract transcribed in plain loops and
against a brute force over every composite path; with ln_switch = -inf the single-model Viterbi restatement; the sanity of
the definition on a planted stream; the argument checks of e2vq_hmm_segment / e2vq_hmm_segment_files and of the CLI, which
run before any HIP call and write no file; the CSV and stdout block of e2vq_hmm_segment_report on a hand-made segmentation;
the exports and the usage text; the kernels' compiler metadata.  The GPU parity tests are in test_gpu_hmm_segment.py."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_segment_restatement as R
from . import hmm_viterbi_restatement as V
from . import lpc_wavs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXE = os.path.join(CSRC, "ecoz2")
NINF = float("-inf")


def _err():
    return e.lib.e2vq_last_error().decode()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _uniform(N, M):
    return np.full(N, 1.0 / N), np.full((N, N), 1.0 / N), np.full((N, M), 1.0 / M)


def _random(rng, N, M, zeros=0.0):
    """rows drawn at random; `zeros`: the share of entries of pi and A set to 0 (a row keeps at least one entry)"""
    def rows(n, m, z):
        x = rng.uniform(0.05, 1.0, (n, m))
        if z:
            x[rng.uniform(size=(n, m)) < z] = 0.0
            x[np.arange(n), rng.integers(0, m, n)] += 0.5
        return x / x.sum(axis=1, keepdims=True)
    return rows(1, N, zeros)[0], rows(N, N, zeros), rows(N, M, 0.0)


def _models(kind, Ns, M, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return [_random(rng, N, M) for N in Ns]
    if kind == "zeros":
        return [_random(rng, N, M, 0.5) for N in Ns]
    if kind == "uniform":
        return [_uniform(N, M) for N in Ns]
    e.hmm.set_random_seed(seed)
    return [hmm.init_model(N, M, 2 if kind == "cascade2" else 3) for N in Ns]


# ---- restatement == transcription ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "zeros", "uniform", "cascade2", "cascade3"])
@pytest.mark.parametrize("Ns", [(1,), (3,), (1, 1), (2, 3, 3, 1), (4, 4, 4)])
def test_restatement_equals_the_transcription(kind, Ns):
    M = 5
    models = _models(kind, Ns, M, 11)
    lms = [V.log_model(*m) for m in models]
    rng = np.random.default_rng(len(Ns))
    for T in (0, 1, 2, 7, 40):
        seq = rng.integers(0, M, T)
        for ls in (NINF, -20.0, -3.0, -0.5, 0.0):
            got = R.segment_logs(lms, seq, ls)
            cls, state, entered, G, lp, st = R.transcribe(models, seq, ls)
            assert got["cls"].tolist() == cls and got["state"].tolist() == state and got["entered"].tolist() == entered
            assert np.array_equal(_bits(got["gbest"]), _bits(G)) and _bits(got["log_prob"]) == _bits(lp) and got["status"] == st
    got = R.segment_logs(lms, [1, M, 2], -1.0)
    assert (got["cls"].tolist(), got["state"].tolist(), got["entered"].tolist(), got["gbest"].tolist(), got["log_prob"], got["status"]) == \
        R.transcribe(models, [1, M, 2], -1.0)
    assert got["status"] == 2 and got["gbest"].tolist() == [0.0, NINF, NINF]


# ---- brute force over every composite path ---------------------------------------------------------------------------
def _brute(lms, seq, ls):
    """the maximum over every path -- per frame t >= 1 a (class, state) and whether it was entered or reached by staying
    in the class -- of the score summed left to right in the contract's order"""
    states = [(k, j) for k, (lpi, _a, _b) in enumerate(lms) for j in range(len(lpi))]
    best = None
    T = len(seq)
    for first in states:
        for tail in itertools.product([(s, how) for s in states for how in ("stay", "enter")], repeat=T - 1):
            k, j = first
            sc = lms[k][0][j] + lms[k][2][j, seq[0]]
            ok = True
            for t, ((k2, j2), how) in enumerate(tail, start=1):
                if how == "stay":
                    if k2 != k:
                        ok = False
                        break
                    sc = (sc + lms[k][1][j, j2]) + lms[k][2][j2, seq[t]]
                else:
                    sc = ((sc + ls) + lms[k2][0][j2]) + lms[k2][2][j2, seq[t]]
                k, j = k2, j2
            if ok and (best is None or sc > best):
                best = sc
    return best


def _rescore(lms, seq, ls, r):
    k, j = int(r["cls"][0]), int(r["state"][0])
    sc = lms[k][0][j] + lms[k][2][j, seq[0]]
    for t in range(1, len(seq)):
        k2, j2 = int(r["cls"][t]), int(r["state"][t])
        if r["entered"][t]:
            sc = ((sc + ls) + lms[k2][0][j2]) + lms[k2][2][j2, seq[t]]
        else:
            assert k2 == k
            sc = (sc + lms[k][1][j, j2]) + lms[k][2][j2, seq[t]]
        k, j = k2, j2
    return sc


@pytest.mark.parametrize("kind", ["random", "zeros", "uniform", "cascade2"])
@pytest.mark.parametrize("Ns", [(1,), (2,), (1, 1), (2, 1), (2, 2), (1, 2, 1)])
def test_brute_force_over_every_composite_path(kind, Ns):
    M = 3
    lms = [V.log_model(*m) for m in _models(kind, Ns, M, 5)]
    rng = np.random.default_rng(sum(Ns))
    for T in (1, 2, 3, 4, 5):
        seq = rng.integers(0, M, T)
        for ls in (NINF, -4.0, -0.25, 0.0):
            r = R.segment_logs(lms, seq, ls)
            with np.errstate(invalid="ignore"):
                want = _brute(lms, seq, ls)
            assert _bits(r["log_prob"]) == _bits(want), (T, ls)
            assert _bits(_rescore(lms, seq, ls, r)) == _bits(want), (T, ls)


# ---- ln_switch = -inf: the best single model ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "uniform", "cascade3"])
def test_without_switching_the_best_single_model_wins(kind):
    M = 6
    Ns = (3, 5, 3, 5)
    models = _models(kind, Ns, M, 3)
    if kind == "random":
        models[3] = models[1]  # two classes reach the maximum: the lower one is reported
    lms = [V.log_model(*m) for m in models]
    rng = np.random.default_rng(8)
    for T in (1, 2, 30, 200):
        seq = rng.integers(0, M, T)
        r = R.segment_logs(lms, seq, NINF)
        single = [V.viterbi_logs(*lm, seq) for lm in lms]
        lps = [s[1] for s in single]
        k = int(np.argmax(lps))
        assert _bits(r["log_prob"]) == _bits(lps[k])
        assert r["cls"].tolist() == [k] * T and r["state"].tolist() == single[k][0].tolist()
        assert r["entered"].tolist() == [1] + [0] * (T - 1)


# ---- sanity of the definition: a planted stream -----------------------------------------------------------------------
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
    sym, truth = [], []
    for k, n in PLANTED:
        pi, A, B = models[k]
        j = rng.choice(len(pi), p=pi)
        for _ in range(n):
            sym.append(rng.choice(B.shape[1], p=B[j]))
            truth.append(k)
            j = rng.choice(len(pi), p=A[j])
    return np.array(sym, dtype=np.uint16), np.array(truth)


def _runs(cls):
    return 1 + int(np.count_nonzero(np.diff(np.asarray(cls, dtype=np.int64))))


@pytest.mark.parametrize("ls", [-5.0, -10.0, -20.0])
def test_a_planted_stream_is_recovered(ls):
    models = planted_models()
    sym, truth = planted_stream(models, np.random.default_rng(3))
    r = R.segment_logs([V.log_model(*m) for m in models], sym, ls)
    acc = float(np.mean(r["cls"] == truth))
    print(f"ln_switch {ls}: {_runs(r['cls'])} class runs, frame accuracy {acc:.4f}")
    assert _runs(r["cls"]) == 5 and acc >= 0.95


def test_without_a_penalty_the_planted_stream_shatters():
    models = planted_models()
    sym, _truth = planted_stream(models, np.random.default_rng(3))
    r = R.segment_logs([V.log_model(*m) for m in models], sym, 0.0)
    print(f"ln_switch 0: {_runs(r['cls'])} class runs")
    assert _runs(r["cls"]) > 50  # (why a penalty is required)


# ---- e2vq_hmm_segment: refusals before the device -----------------------------------------------------------------------
def _segment_c(models, ln_switch, Ns=None, K=None):
    Ns = [len(m[0]) for m in models] if Ns is None else Ns
    K = len(models) if K is None else K
    n = max(len(models), 1)
    ns = (C.c_int * n)(*Ns)
    keep = [[np.ascontiguousarray(m[i], dtype=np.float64) for m in models] for i in range(3)]
    ptr = lambda i: (C.c_void_p * n)(*[a.ctypes.data for a in keep[i]])
    sym, offs = np.zeros(8, np.uint16), np.array([0, 8], np.int64)
    return e.lib.e2vq_hmm_segment(0, K, ns, 8, ptr(0), ptr(1), ptr(2), sym.ctypes.data, offs.ctypes.data, 1, ln_switch,
                                  *([None] * 6), 0)


def _bad(where, value):
    pi, A, B = (x.copy() for x in _uniform(3, 8))
    {"pi": pi, "A": A, "B": B}[where].flat[1] = value
    return pi, A, B


@pytest.mark.parametrize("case,needle", [
    ("K0", "e2vq_hmm_segment: 0 models (at least 1)"),
    ("N0", "e2vq_hmm_segment: model 1 has N=0 states (1 .. 64)"),
    ("N65", "e2vq_hmm_segment: model 0 has N=65 states (1 .. 64)"),
    ("sumN", "e2vq_hmm_segment: 4160 states in all models (at most 4096)"),
    ("negative", "HMM parameter A[1] = -0.25: not a finite non-negative number"),
    ("nan", "HMM parameter pi[1] = nan: not a finite non-negative number"),
    ("inf", "HMM parameter B[1] = inf: not a finite non-negative number"),
    ("switch_nan", "e2vq_hmm_segment: ln_switch = nan"),
    ("switch_pos", "e2vq_hmm_segment: ln_switch = 0.5"),
])
def test_segment_refuses_before_the_device(case, needle):
    ok = _uniform(3, 8)
    if case == "K0":
        rc = _segment_c([ok], -1.0, K=0)
    elif case == "N0":
        rc = _segment_c([ok, ok], -1.0, Ns=[3, 0])
    elif case == "N65":
        rc = _segment_c([_uniform(65, 8)], -1.0)
    elif case == "sumN":
        rc = _segment_c([_uniform(64, 8)] * 65, -1.0)
    elif case == "negative":
        rc = _segment_c([ok, _bad("A", -0.25)], -1.0)
    elif case == "nan":
        rc = _segment_c([_bad("pi", float("nan"))], -1.0)
    elif case == "inf":
        rc = _segment_c([_bad("B", float("inf"))], -1.0)
    elif case == "switch_nan":
        rc = _segment_c([ok], float("nan"))
    else:
        rc = _segment_c([ok], 0.5)
    assert rc == 1 and needle in _err(), _err()


def test_python_mirror_raises_the_refusal():
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment([_uniform(3, 8)], np.zeros(8, np.uint16), [0, 8], 1.0)
    assert "ln_switch = 1" in str(ei.value)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment([], np.zeros(8, np.uint16), [0, 8], -1.0)
    assert "0 models (at least 1)" in str(ei.value)


# ---- e2vq_hmm_segment_files and the CLI: refusals ---------------------------------------------------------------------------
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
    (d / "many").mkdir()
    for k in range(65):
        hmm.save_model(d / "many" / f"c{k:02d}.hmm", f"c{k:02d}", *_uniform(64, 16))
    rng = np.random.default_rng(1)
    e.formats.write_cbook(str(d / "m16p4.cbook"), "_", rng.uniform(-0.5, 0.5, (16, 5)))
    e.formats.write_cbook(str(d / "m32p4.cbook"), "_", rng.uniform(-0.5, 0.5, (32, 5)))
    e.formats.write_cbook(str(d / "m16p6.cbook"), "_", rng.uniform(-0.5, 0.5, (16, 7)))
    e.formats.write_prd(str(d / "x.prd"), "A", rng.uniform(0.1, 1.0, (40, 5)))
    e.formats.write_seq(str(d / "x.seq"), "A", 16, np.arange(40) % 16)
    e.formats.write_seq(str(d / "y32.seq"), "A", 32, np.arange(40) % 32)
    lpc_wavs.write_wav(d / "x.wav", lpc_wavs.to_pcm(lpc_wavs.ar_source(3, 4, 4000, 0.5), 16), 8000, 16)
    (d / "notes.txt").write_text("x")
    return tmp_path, d, models


def _segment_files(models, inputs, out, codebook=None, P=4, ls=-5.0):
    m, _k1 = hmm._strs(models)
    f, _k2 = hmm._strs(inputs)
    return e.lib.e2vq_hmm_segment_files(m, len(models), str(codebook).encode() if codebook else None, f, len(inputs), P, 45, 15, ls,
                                        str(out).encode())


@pytest.mark.parametrize("case,needle", [
    ("no_models", "e2vq_hmm_segment_files: no models"),
    ("no_inputs", "e2vq_hmm_segment_files: no inputs"),
    ("switch_pos", "e2vq_hmm_segment_files: ln_switch = 2"),
    ("switch_nan", "e2vq_hmm_segment_files: ln_switch = nan"),
    ("N65", "e2vq_hmm_segment_files: model 2 has N=65 states (1 .. 64)"),
    ("sumN", "e2vq_hmm_segment_files: 4160 states in all models (at most 4096)"),
    ("models_M", "model has M=32 but"),
    ("cb_M", "codebook has M=32 but the models have M=16"),
    ("cb_P_prd", "x.prd: prediction order 4 differs from the codebook's 6"),
    ("cb_P_wav", "x.wav: prediction order -P 4 differs from the codebook's 6"),
    ("seq_M", "y32.seq: codebook size 32 differs from the models' 16"),
    ("no_codebook", "e2vq_hmm_segment_files: signals and predictors need a codebook"),
    ("extension", "notes.txt: not a .wav, .prd or .seq file"),
    ("same_csv", "would both write"),
])
def test_segment_files_refuses_before_the_device(corpus, case, needle):
    tmp_path, d, models = corpus
    kw = dict(codebook=d / "m16p4.cbook")
    inputs = [str(d / "x.seq")]
    if case == "no_models":
        models = []
    elif case == "no_inputs":
        inputs = []
    elif case == "switch_pos":
        kw["ls"] = 2.0
    elif case == "switch_nan":
        kw["ls"] = float("nan")
    elif case == "N65":
        models = models + [str(d / "N65.hmm")]
    elif case == "sumN":
        models = [str(d / "many" / f"c{k:02d}.hmm") for k in range(65)]
    elif case == "models_M":
        models = models + [str(d / "C32.hmm")]
    elif case == "cb_M":
        kw["codebook"] = d / "m32p4.cbook"
        inputs = [str(d / "x.prd")]
    elif case == "cb_P_prd":
        kw["codebook"] = d / "m16p6.cbook"
        inputs = [str(d / "x.prd")]
    elif case == "cb_P_wav":
        kw["codebook"] = d / "m16p6.cbook"
        inputs = [str(d / "x.wav")]
    elif case == "seq_M":
        inputs = [str(d / "x.seq"), str(d / "y32.seq")]
    elif case == "no_codebook":
        kw["codebook"] = None
        inputs = [str(d / "x.prd")]
    elif case == "extension":
        inputs = [str(d / "notes.txt")]
    else:
        inputs = [str(d / "x.seq"), str(d / "x.prd")]
    out = tmp_path / "out"
    assert _segment_files(models, inputs, out, **kw) == 1
    assert needle in _err(), _err()
    assert not out.exists()


def test_segment_files_refuses_a_bad_parameter(corpus):
    tmp_path, d, models = corpus
    pi, A, B = _uniform(3, 16)
    A[1, 2] = -1.0
    hmm.save_model(d / "bad.hmm", "bad", pi, A, B)
    assert _segment_files(models + [str(d / "bad.hmm")], [str(d / "x.seq")], tmp_path / "out") == 1
    assert "bad.hmm: HMM parameter A[5] = -1: not a finite non-negative number" in _err(), _err()


def _cli(cwd, *args):
    r = subprocess.run([EXE, "hmm", "segment", *args], cwd=cwd, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("args,code,needle", [
    (["--sequences", "in/x.seq", "--switch-penalty", "-5"], 2, "hmm segment: --models <files|dirs>... is required"),
    (["--models", "in/A.hmm", "--switch-penalty", "-5"], 2, "hmm segment: exactly one of --signals, --predictors and --sequences"),
    (["--models", "in/A.hmm", "--switch-penalty", "-5", "--sequences", "in/x.seq", "--predictors", "in/x.prd"], 2, "exactly one of"),
    (["--models", "in/A.hmm", "--sequences", "in/x.seq"], 2, "hmm segment: --switch-penalty <x <= 0 | -inf> is required"),
    (["--models", "in/A.hmm", "--sequences", "in/x.seq", "--switch-penalty", "3"], 2, "--switch-penalty 3: at most 0"),
    (["--models", "in/A.hmm", "--sequences", "in/x.seq", "--switch-penalty", "nan"], 2, "--switch-penalty nan: at most 0"),
    (["--models", "in/A.hmm", "--sequences", "in/x.seq", "--switch-penalty", "soon"], 2, "--switch-penalty: invalid value 'soon'"),
    (["--models", "in/A.hmm", "--signals", "in/x.wav", "--switch-penalty", "-5"], 2, "--signals and --predictors need --codebook"),
    (["--models", "in/A.hmm", "in/C32.hmm", "--sequences", "in/x.seq", "--switch-penalty", "-5", "-c", "out"], 1, "model has M=32 but"),
    (["--models", "in/A.hmm", "in/N65.hmm", "--sequences", "in/x.seq", "--switch-penalty", "-inf", "-c", "out"], 1,
     "model 1 has N=65 states (1 .. 64)"),
    (["--models", "in/many", "--sequences", "in/x.seq", "--switch-penalty", "-5", "-c", "out"], 1, "4160 states in all models"),
    (["--models", "in/A.hmm", "--sequences", "in/y32.seq", "--switch-penalty", "-5", "-c", "out"], 1,
     "codebook size 32 differs from the models' 16"),
])
def test_cli_refusals(corpus, args, code, needle):
    tmp_path, _d, _models = corpus
    rc, out, err = _cli(tmp_path, *args)
    assert rc == code and needle in (err if code == 2 else out), (rc, out, err)
    assert not (tmp_path / "out").exists()


def test_usage_names_hmm_segment(tmp_path):
    rc, _out, err = _cli(tmp_path)
    assert rc == 2 and "ecoz2 hmm segment -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15]" in err
    assert "--switch-penalty <x <= 0 | -inf> [-c <csv dir|file.csv>]" in err


# ---- the report: CSV and stdout block of a hand-made segmentation ---------------------------------------------------------
def _report(tmp_path, capfd, cls, entered, gbest, lp, ls, names=("whale", "noise", "ship")):
    names_c, _k = hmm._strs(names)
    cls, entered, gbest = np.array(cls, np.uint16), np.array(entered, np.uint8), np.array(gbest, np.float64)
    csv = tmp_path / "rep" / "x.csv"
    capfd.readouterr()
    rc = e.lib.e2vq_hmm_segment_report(b"x.wav", len(cls), len(names), names_c, 45, 15, cls.ctypes.data, entered.ctypes.data,
                                       gbest.ctypes.data, lp, ls, str(csv).encode())
    assert rc == 0, _err()
    return csv.read_text().split("\n"), capfd.readouterr().out.split("\n")


def test_report_csv_and_block(tmp_path, capfd):
    g = lambda x: "%.17g" % x
    cls = [0, 0, 0, 1, 1, 1, 1, 1, 2, 2]
    entered = [1, 0, 0, 1, 0, 1, 0, 0, 1, 0]  # two adjacent segments of `noise`: [3, 5) and [5, 8)
    gbest = [0.0, -1.0, -3.0, -6.0, -9.0, -13.5, -15.0, -19.0, -22.25, -26.0]
    rows, out = _report(tmp_path, capfd, cls, entered, gbest, -30.0, -2.0)
    assert rows[0] == "segment,begin_frame,end_frame,begin_s,end_s,class,log_prob,log_prob_per_frame"
    assert rows[1] == f"0,0,3,0,{g(0.075)},whale,-6,-2"
    assert rows[2] == f"1,3,5,{g(0.045)},{g(0.105)},noise,-5.5,-2.75"            # -13.5 - (-6 - 2)
    assert rows[3] == f"2,5,8,{g(0.075)},{g(0.15)},noise,-6.75,-2.25"            # -22.25 - (-13.5 - 2)
    assert rows[4] == f"3,8,10,{g(0.12)},{g(0.18)},ship,-5.75,-2.875"            # -30 - (-22.25 - 2)
    assert rows[5] == "" and len(rows) == 6
    assert out[0] == "x.wav: T=10  segments=4  (switch penalty -2)"
    assert out[1:4] == ["  'whale': 3", "  'noise': 5", "  'ship': 2"]
    assert out[4] == "  segments:"
    assert out[5:9] == ["    0.000 - 0.075 whale", "    0.045 - 0.105 noise", "    0.075 - 0.150 noise", "    0.120 - 0.180 ship"]
    assert out[9].endswith("x.csv saved")
    # the same arithmetic in the Python mirror
    segs = hmm.segments_of(np.array(cls), np.array(entered), np.array(gbest), -30.0, -2.0)
    assert [(s["begin"], s["end"], s["cls"], s["log_prob"]) for s in segs] == \
        [(0, 3, 0, -6.0), (3, 5, 1, -5.5), (5, 8, 1, -6.75), (8, 10, 2, -5.75)]


def test_report_of_a_single_segment_and_of_an_empty_stream(tmp_path, capfd):
    rows, out = _report(tmp_path, capfd, [1] * 4, [1, 0, 0, 0], [0.0, -1.0, -2.0, -2.5], -3.0, NINF)
    assert rows[1] == "0,0,4,0,0.089999999999999997,noise,-3,-0.75" and rows[2] == "" and len(rows) == 3
    assert out[0] == "x.wav: T=4  segments=1  (switch penalty -inf)" and out[5] == "    0.000 - 0.090 noise"
    rows, out = _report(tmp_path, capfd, [], [], [], 0.0, -1.0)
    assert rows == ["segment,begin_frame,end_frame,begin_s,end_s,class,log_prob,log_prob_per_frame", ""]
    assert out[0] == "x.wav: T=0  segments=0  (switch penalty -1)"


def test_report_refuses_what_is_no_segmentation(tmp_path):
    names_c, _k = hmm._strs(["a"])
    g = np.zeros(2)
    for cls, entered, needle in (([0, 1], [1, 0], "frame 1 names a model outside [0, 1)"), ([0, 0], [0, 1], "frame 0 does not start")):
        cls, entered = np.array(cls, np.uint16), np.array(entered, np.uint8)
        rc = e.lib.e2vq_hmm_segment_report(b"x", 2, 1, names_c, 45, 15, cls.ctypes.data, entered.ctypes.data, g.ctypes.data, -1.0, -1.0,
                                           str(tmp_path / "no.csv").encode())
        assert rc == 1 and needle in _err(), _err()
    assert not (tmp_path / "no.csv").exists()


def test_segment_library_exports():
    for name in ("e2vq_hmm_segment", "e2vq_hmm_segment_files", "e2vq_hmm_segment_report", "e2vq_hmm_segment_last_kernel_ms"):
        assert hasattr(e.lib, name)
    assert callable(hmm.segment) and callable(hmm.segment_files) and callable(hmm.segment_last_kernel_ms)


# ---- compiler metadata (read as test_hmm_scan_cpu.py reads its kernels') ------------------------------------------------------
VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_segment.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_segment.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _meta(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    return lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))


@pytest.mark.parametrize("pattern", [r"k_hmm_segmentILb0ELb0E", r"k_hmm_segmentILb0ELb1E", r"k_hmm_segmentILb1ELb0E",
                                     r"k_hmm_segmentILb1ELb1E", r"k_hmm_segment_backtrackE"])
def test_segment_kernels_have_no_scratch_no_spill_and_fit_their_budget(asm, pattern):
    g = _meta(asm, pattern)
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
