"""`hmm segment --class-transitions`, CPU side: the numpy restatement against the contract transcribed in
plain loops and against a brute force over every composite path; the uniform matrix against the restatement of `hmm segment`;
forbidden successions; the argument checks of e2vq_hmm_segment_trans / e2vq_hmm_segment_trans_files and of the CLI, which run
before any HIP call and write no file; the transitions file; the report on a hand-made segmentation; the estimator of the
matrix; the exports and the usage text; the kernels' compiler metadata.  The GPU parity tests are in
test_gpu_hmm_segment_trans.py."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_segment_restatement as R
from . import hmm_segment_trans_cases as cases
from . import hmm_segment_trans_restatement as RT
from . import hmm_viterbi_restatement as V

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


def _models(kind, Ns, M, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return [cases.random_model(rng, N, M) for N in Ns]
    if kind == "zeros":
        return [cases.random_model(rng, N, M, 0.5) for N in Ns]
    if kind == "uniform":
        return [_uniform(N, M) for N in Ns]
    e.hmm.set_random_seed(seed)
    return [hmm.init_model(N, M, 2 if kind == "cascade2" else 3) for N in Ns]


def _same(got, want):
    cls, state, entered, ex, lp, st = want
    return (got["cls"].tolist() == cls and got["state"].tolist() == state and got["entered"].tolist() == entered and
            np.array_equal(_bits(got["exit_score"]), _bits(ex)) and _bits(got["log_prob"]) == _bits(lp) and got["status"] == st)


# ---- restatement == transcription ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "zeros", "uniform", "cascade2", "cascade3"])
@pytest.mark.parametrize("Ns", [(1,), (3,), (1, 1), (2, 3, 3, 1), (4, 4, 4)])
def test_restatement_equals_the_transcription(kind, Ns):
    M, K = 5, len(Ns)
    models = _models(kind, Ns, M, 11)
    lms = [V.log_model(*m) for m in models]
    rng = np.random.default_rng(K)
    for T in (0, 1, 2, 7, 40):
        seq = rng.integers(0, M, T)
        for lt in (cases.random_prices(rng, K), cases.random_prices(rng, K, 0.6), np.full((K, K), NINF), np.zeros((K, K))):
            assert _same(RT.segment_trans_logs(lms, seq, lt), RT.transcribe(models, seq, lt)), (T, lt)
    lt = cases.random_prices(rng, K)
    got = RT.segment_trans_logs(lms, [1, M, 2], lt)
    assert _same(got, RT.transcribe(models, [1, M, 2], lt))
    assert got["status"] == 2 and got["exit_score"].tolist() == [0.0, NINF, NINF]


# ---- brute force over every composite path ---------------------------------------------------------------------------
def _brute(lms, seq, lt):
    """the maximum over every path -- per frame t >= 1 a (class, state) and whether it was entered or reached by staying in
    the class -- of the score summed left to right in the contract's order, the number of paths reaching it, and one of them"""
    states = [(k, j) for k, (lpi, _a, _b) in enumerate(lms) for j in range(len(lpi))]
    best, count, path = None, 0, None
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
                    sc = ((sc + lt[k][k2]) + lms[k2][0][j2]) + lms[k2][2][j2, seq[t]]
                k, j = k2, j2
            if not ok:
                continue
            if best is None or sc > best:
                best, count, path = sc, 1, (first, tail)
            elif sc == best:
                count += 1
    return best, count, path


def _rescore(lms, seq, lt, r):
    k, j = int(r["cls"][0]), int(r["state"][0])
    sc = lms[k][0][j] + lms[k][2][j, seq[0]]
    for t in range(1, len(seq)):
        k2, j2 = int(r["cls"][t]), int(r["state"][t])
        if r["entered"][t]:
            sc = ((sc + lt[k][k2]) + lms[k2][0][j2]) + lms[k2][2][j2, seq[t]]
        else:
            assert k2 == k
            sc = (sc + lms[k][1][j, j2]) + lms[k][2][j2, seq[t]]
        k, j = k2, j2
    return sc


@pytest.mark.parametrize("kind", ["random", "zeros", "cascade2"])
@pytest.mark.parametrize("Ns", [(1,), (2,), (1, 1), (2, 1), (2, 2), (1, 2, 1), (2, 1, 2)])
def test_brute_force_over_every_composite_path(kind, Ns):
    M, K = 3, len(Ns)
    lms = [V.log_model(*m) for m in _models(kind, Ns, M, 5)]
    rng = np.random.default_rng(sum(Ns))
    unique = 0
    for T in (1, 2, 3, 4, 5) if sum(Ns) < 5 else (1, 2, 3, 4):
        seq = rng.integers(0, M, T)
        for lt in (cases.random_prices(rng, K, 0.0), cases.random_prices(rng, K, 0.4)):
            r = RT.segment_trans_logs(lms, seq, lt)
            with np.errstate(invalid="ignore"):
                want, count, path = _brute(lms, seq, lt)
                assert _bits(r["log_prob"]) == _bits(want), (T, lt)
                assert _bits(_rescore(lms, seq, lt, r)) == _bits(want), (T, lt)
            if count == 1 and want > NINF:
                unique += 1
                first, tail = path
                assert list(zip(r["cls"].tolist(), r["state"].tolist())) == [first] + [s for s, _how in tail]
                assert r["entered"].tolist() == [1] + [1 if how == "enter" else 0 for _s, how in tail]
    assert unique > 0 or kind != "random"


# ---- the uniform matrix: `hmm segment` ---------------------------------------------------------------------------------
def _segment_d(models, seq, ls):
    """d_t of DESIGN.md 4.8.6, literally (tests/hmm_segment_restatement.py keeps only the path)"""
    lms = [V.log_model(*m) for m in models]
    d = [[float(lpi[j] + lB[j, seq[0]]) for j in range(len(lpi))] for lpi, _lA, lB in lms]
    out = [d]
    for t in range(1, len(seq)):
        G = max(x for row in d for x in row)
        base = G + ls
        nd = []
        for k, (lpi, lA, lB) in enumerate(lms):
            row = []
            for j in range(len(lpi)):
                best = d[k][0] + lA[0, j]
                for i in range(1, len(lpi)):
                    v = d[k][i] + lA[i, j]
                    if v > best:
                        best = v
                x = base + lpi[j]
                if x > best:
                    best = x
                row.append(float(best + lB[j, seq[t]]))
            nd.append(row)
        d = nd
        out.append(d)
    return out


def _assert_uniform_is_segment(models, seq, ls):
    K = len(models)
    lt = np.full((K, K), ls)
    lms = [V.log_model(*m) for m in models]
    u, r = RT.segment_trans_logs(lms, seq, lt), R.segment_logs(lms, seq, ls)
    # (the paths could differ only where two different E_t[f] round to the same sum: an input that does would be replaced)
    assert u["cls"].tolist() == r["cls"].tolist() and u["state"].tolist() == r["state"].tolist()
    assert u["entered"].tolist() == r["entered"].tolist() and u["status"] == r["status"]
    assert _bits(u["log_prob"]) == _bits(r["log_prob"])
    at = np.flatnonzero(r["entered"])
    assert np.array_equal(_bits(u["exit_score"][at]), _bits(r["gbest"][at]))
    a, b = RT.segments_of(u["cls"], u["entered"], u["exit_score"], u["log_prob"], lt), R.segments_of(r["cls"], r["entered"], r["gbest"], r["log_prob"], ls)
    assert [x[:3] for x in a] == [x[:3] for x in b] and np.array_equal(_bits([x[3] for x in a]), _bits([x[3] for x in b]))
    return u


@pytest.mark.parametrize("case", [c[0] for c in cases.uniform_cases()])
def test_the_shared_uniform_cases_agree_between_the_restatements(case):
    _name, models, streams = next(c for c in cases.uniform_cases() if c[0] == case)
    for seq in streams:
        _assert_uniform_is_segment(models, seq, cases.UNIFORM_PRICE)


@pytest.mark.parametrize("ls", [0.0, -0.5, -5.0, -20.0, NINF])
def test_a_uniform_matrix_is_hmm_segment(ls):
    rng = np.random.default_rng(17)
    for it in range(8):
        K = int(rng.integers(1, 7))
        Ns = rng.integers(1, 7, K)
        M = 6
        models = [cases.random_model(rng, int(N), M, 0.4 if it % 2 else 0.0) for N in Ns]
        if K > 2 and it % 3 == 0:
            models[-1] = models[0]  # a duplicated class: exact ties between the sources
        seq = rng.integers(0, M, int(rng.integers(1, 120)))
        _assert_uniform_is_segment(models, seq, ls)
        if it < 3:  # d itself, bit for bit
            ds = RT.transcribe(models, seq, np.full((K, K), ls), want_d=True)[6]
            want = _segment_d(models, seq, ls)
            assert all(np.array_equal(_bits(sum(a, [])), _bits(sum(b, []))) for a, b in zip(ds, want)) and len(ds) == len(want)


# ---- forbidden successions -----------------------------------------------------------------------------------------------
def test_forbidden_pairs_never_occur_and_without_any_pair_the_best_single_model_wins():
    M, Ns = 6, (3, 5, 3, 4)
    K = len(Ns)
    rng = np.random.default_rng(3)
    models = [cases.random_model(rng, N, M) for N in Ns]
    lms = [V.log_model(*m) for m in models]
    seen = 0
    for T in (2, 30, 200):
        seq = rng.integers(0, M, T)
        free = RT.segment_trans_logs(lms, seq, np.full((K, K), -0.5))
        # forbid what the unconstrained decode likes best
        pairs = {(int(free["cls"][t - 1]), int(free["cls"][t])) for t in range(1, T) if free["entered"][t]}
        pairs |= {(0, 0), (1, 3)}
        lt = np.full((K, K), -0.5)
        for f, k in pairs:
            lt[f, k] = NINF
        r = RT.segment_trans_logs(lms, seq, lt)
        assert r["status"] == 0
        got = {(int(r["cls"][t - 1]), int(r["cls"][t])) for t in range(1, T) if r["entered"][t]}
        assert not (got & pairs)
        seen += len(got)
        r = RT.segment_trans_logs(lms, seq, np.full((K, K), NINF))
        single = [V.viterbi_logs(*lm, seq) for lm in lms]
        k = int(np.argmax([s[1] for s in single]))
        assert _bits(r["log_prob"]) == _bits(single[k][1])
        assert r["cls"].tolist() == [k] * T and r["state"].tolist() == single[k][0].tolist() and r["entered"].tolist() == [1] + [0] * (T - 1)
    assert seen > 0  # (the constrained decodes still switch: the property was exercised)


# ---- e2vq_hmm_segment_trans: refusals before the device -------------------------------------------------------------------
def _segment_trans_c(models, lt, Ns=None, K=None):
    Ns = [len(m[0]) for m in models] if Ns is None else Ns
    K = len(models) if K is None else K
    n = max(len(models), 1)
    ns = (C.c_int * n)(*Ns)
    keep = [[np.ascontiguousarray(m[i], dtype=np.float64) for m in models] for i in range(3)]
    ptr = lambda i: (C.c_void_p * n)(*[a.ctypes.data for a in keep[i]])
    sym, offs = np.zeros(8, np.uint16), np.array([0, 8], np.int64)
    lt = np.ascontiguousarray(lt, dtype=np.float64)
    return e.lib.e2vq_hmm_segment_trans(0, K, ns, 8, ptr(0), ptr(1), ptr(2), sym.ctypes.data, offs.ctypes.data, 1, lt.ctypes.data,
                                        *([None] * 6), 0)


def _bad(where, value):
    pi, A, B = (x.copy() for x in _uniform(3, 8))
    {"pi": pi, "A": A, "B": B}[where].flat[1] = value
    return pi, A, B


@pytest.mark.parametrize("case,needle", [
    ("K0", "e2vq_hmm_segment_trans: 0 models (at least 1)"),
    ("N0", "e2vq_hmm_segment_trans: model 1 has N=0 states (1 .. 64)"),
    ("N65", "e2vq_hmm_segment_trans: model 0 has N=65 states (1 .. 64)"),
    ("sumN", "e2vq_hmm_segment_trans: 4160 states in all models (at most 4096)"),
    ("negative", "HMM parameter A[1] = -0.25: not a finite non-negative number"),
    ("nan", "HMM parameter pi[1] = nan: not a finite non-negative number"),
    ("lt_nan", "e2vq_hmm_segment_trans: lt[1][0] = nan: the logarithm of a price, at most 0"),
    ("lt_pos", "e2vq_hmm_segment_trans: lt[0][1] = 0.5: the logarithm of a price, at most 0"),
    ("slots17", "e2vq_hmm_segment_trans: the classes take 17 wave-slots of 64 lanes (at most 16"),
    ("slots_packed", "e2vq_hmm_segment_trans: the classes take 17 wave-slots of 64 lanes (at most 16"),
])
def test_segment_trans_refuses_before_the_device(case, needle):
    ok = _uniform(3, 8)
    z = lambda K: np.zeros((K, K))
    if case == "K0":
        rc = _segment_trans_c([ok], z(1), K=0)
    elif case == "N0":
        rc = _segment_trans_c([ok, ok], z(2), Ns=[3, 0])
    elif case == "N65":
        rc = _segment_trans_c([_uniform(65, 8)], z(1))
    elif case == "sumN":
        rc = _segment_trans_c([_uniform(64, 8)] * 65, z(65))
    elif case == "negative":
        rc = _segment_trans_c([ok, _bad("A", -0.25)], z(2))
    elif case == "nan":
        rc = _segment_trans_c([_bad("pi", float("nan"))], z(1))
    elif case == "lt_nan":
        rc = _segment_trans_c([ok, ok], [[0.0, -1.0], [float("nan"), 0.0]])
    elif case == "lt_pos":
        rc = _segment_trans_c([ok, ok], [[0.0, 0.5], [-1.0, NINF]])
    elif case == "slots17":
        rc = _segment_trans_c([_uniform(64, 8)] * 17, z(17))
    else:
        rc = _segment_trans_c([_uniform(33, 8)] * 17, z(17))  # (two classes of 33 states do not share a slot)
    assert rc == 1 and needle in _err(), _err()


def test_python_mirror_raises_the_refusal():
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment_trans([_uniform(3, 8)], np.zeros(8, np.uint16), [0, 8], [[1.0]])
    assert "lt[0][0] = 1" in str(ei.value)
    with pytest.raises(ValueError):
        hmm.segment_trans([_uniform(3, 8)], np.zeros(8, np.uint16), [0, 8], np.zeros((2, 2)))


# ---- the transitions file -------------------------------------------------------------------------------------------------
def test_transitions_file_round_trip_in_any_order(tmp_path):
    names = ["rain", "ship", "whale"]
    lt = np.array([[-0.5, NINF, -2.25], [-1e-3, -7.0, NINF], [0.0, -0.1, -3.0]])
    hmm.write_class_transitions(tmp_path / "a" / "t.csv", names, lt)
    text = (tmp_path / "a" / "t.csv").read_text()
    assert text.split("\n")[0] == "class,rain,ship,whale" and text.split("\n")[1] == "rain,-0.5,-inf,-2.25" and text.endswith("\n")
    assert np.array_equal(_bits(hmm.read_class_transitions(tmp_path / "a" / "t.csv", names)), _bits(lt))
    order = [2, 0, 1]
    assert np.array_equal(_bits(hmm.read_class_transitions(tmp_path / "a" / "t.csv", [names[k] for k in order])), _bits(lt[np.ix_(order, order)]))
    (tmp_path / "hand.csv").write_text("class,whale,rain,ship\r\nship,-inf,-1e-3,-7\r\nwhale,-3,0,-0.1\r\nrain,-2.25,-0.5,-INF")
    assert np.array_equal(_bits(hmm.read_class_transitions(tmp_path / "hand.csv", names)), _bits(lt))


@pytest.mark.parametrize("text,needle", [
    ("", "t.csv: empty"),
    ("from,a,b\na,0,0\nb,0,0\n", "t.csv:1: the header starts with 'from', not 'class'"),
    ("class,a\na,0\n", "t.csv:1: 1 class names for 2 models"),
    ("class,a,b,c\na,0,0,0\n", "t.csv:1: 3 class names for 2 models"),
    ("class,a,c\na,0,0\nb,0,0\n", "t.csv:1: 'c' is no model's class"),
    ("class,a,a\na,0,0\nb,0,0\n", "t.csv:1: class 'a' is named twice"),
    ("class,a,b\na,0,0\n", "t.csv:2: 1 rows for 2 models"),
    ("class,a,b\na,0,0\nb,0,0\nb,0,0\n", "t.csv:4: 3 rows for 2 models"),
    ("class,a,b\na,0,0\nb,0\n", "t.csv:3: 2 fields, not 3"),
    ("class,a,b\na,0,0\nc,0,0\n", "t.csv:3: 'c' is no model's class"),
    ("class,a,b\na,0,0\na,0,0\n", "t.csv:3: class 'a' has a second row"),
    ("class,a,b\na,0,-1x\nb,0,0\n", "t.csv:2: '-1x' is not a number"),
    ("class,a,b\na,0,\nb,0,0\n", "t.csv:2: '' is not a number"),
    ("class,a,b\na,0,0\nb,0.25,0\n", "t.csv:3: b -> a = 0.25: the logarithm of a price, at most 0 or -inf"),
    ("class,a,b\na,0,nan\nb,0,0\n", "t.csv:2: a -> b = nan: the logarithm of a price, at most 0 or -inf"),
    ("class,a,b\na,0,inf\nb,0,0\n", "t.csv:2: a -> b = inf"),
])
def test_transitions_file_refusals_name_the_file_and_line(tmp_path, text, needle):
    (tmp_path / "t.csv").write_text(text)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.read_class_transitions(tmp_path / "t.csv", ["a", "b"])
    assert needle in str(ei.value)


def test_a_missing_transitions_file_is_refused(tmp_path):
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.read_class_transitions(tmp_path / "none.csv", ["a"])
    assert "none.csv" in str(ei.value)


# ---- e2vq_hmm_segment_trans_files and the CLI: refusals -------------------------------------------------------------------
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
    (d / "t.csv").write_text("class,A,B\nA,0,-1\nB,-2,-inf\n")
    (d / "t3.csv").write_text("class,A,B,C\nA,0,-1,0\nB,-2,-inf,0\nC,0,0,0\n")
    (d / "tpos.csv").write_text("class,A,B\nA,0,-1\nB,2,-inf\n")
    (d / "notes.txt").write_text("x")
    return tmp_path, d, models


def _trans_files(models, inputs, out, transitions, ls=-5.0):
    m, _k1 = hmm._strs(models)
    f, _k2 = hmm._strs(inputs)
    return e.lib.e2vq_hmm_segment_trans_files(m, len(models), None, f, len(inputs), 4, 45, 15, ls,
                                              str(transitions).encode() if transitions else None, str(out).encode())


@pytest.mark.parametrize("case,needle", [
    ("no_models", "e2vq_hmm_segment_trans_files: no models"),
    ("no_inputs", "e2vq_hmm_segment_trans_files: no inputs"),
    ("no_file", "e2vq_hmm_segment_trans_files: no class-transitions file"),
    ("switch_pos", "e2vq_hmm_segment_trans_files: ln_switch = 2"),
    ("N65", "e2vq_hmm_segment_trans_files: model 2 has N=65 states (1 .. 64)"),
    ("slots", "e2vq_hmm_segment_trans_files: the classes take 17 wave-slots of 64 lanes (at most 16"),
    ("same_class", "e2vq_hmm_segment_trans_files: two models of the class 'A'"),
    ("missing", "none.csv"),
    ("names", "t3.csv:1: 3 class names for 2 models"),
    ("value", "tpos.csv:3: B -> A = 2: the logarithm of a price"),
    ("seq_M", "y32.seq: codebook size 32 differs from the models' 16"),
    ("extension", "notes.txt: not a .wav, .prd or .seq file"),
])
def test_segment_trans_files_refuses_before_the_device(corpus, case, needle):
    tmp_path, d, models = corpus
    inputs, transitions, ls = [str(d / "x.seq")], d / "t.csv", -5.0
    if case == "no_models":
        models = []
    elif case == "no_inputs":
        inputs = []
    elif case == "no_file":
        transitions = None
    elif case == "switch_pos":
        ls = 2.0
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
    else:
        inputs = [str(d / "notes.txt")]
    out = tmp_path / "out"
    assert _trans_files(models, inputs, out, transitions, ls) == 1
    assert needle in _err(), _err()
    assert not out.exists()


def _cli(cwd, *args):
    r = subprocess.run([EXE, "hmm", *args], cwd=cwd, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("args,code,needle", [
    (["--models", "in/A.hmm", "in/B.hmm", "--sequences", "in/x.seq", "--switch-penalty", "-5", "--class-transitions", "in/t.csv",
      "--posteriors"], 2, "hmm segment: --class-transitions and --posteriors exclude one another"),
    (["--models", "in/A.hmm", "in/B.hmm", "--sequences", "in/x.seq", "--class-transitions", "in/t.csv"], 2,
     "hmm segment: --switch-penalty <x <= 0 | -inf> is required"),
    (["--models", "in/A.hmm", "in/B.hmm", "--sequences", "in/x.seq", "--switch-penalty", "-5", "--class-transitions"], 2,
     "--class-transitions needs a value"),
    (["--models", "in/A.hmm", "in/B.hmm", "--sequences", "in/x.seq", "--switch-penalty", "0", "--class-transitions", "in/tpos.csv",
      "-c", "out"], 1, "in/tpos.csv:3: B -> A = 2"),
    (["--models", "in/A.hmm", "in/B.hmm", "--sequences", "in/x.seq", "--switch-penalty", "0", "--class-transitions", "in/t3.csv",
      "-c", "out"], 1, "in/t3.csv:1: 3 class names for 2 models"),
    (["--models", "in/many", "--sequences", "in/x.seq", "--switch-penalty", "-1", "--class-transitions", "in/t.csv", "-c", "out"], 1,
     "the classes take 17 wave-slots of 64 lanes"),
])
def test_cli_refusals(corpus, args, code, needle):
    tmp_path, _d, _models = corpus
    rc, out, err = _cli(tmp_path, "segment", *args)
    assert rc == code and needle in (err if code == 2 else out), (rc, out, err)
    assert not (tmp_path / "out").exists()


def test_usage_names_the_new_option_and_command(tmp_path):
    rc, _out, err = _cli(tmp_path, "segment")
    assert rc == 2 and "                  [--class-transitions <file.csv>]\n" in err
    assert "  ecoz2 hmm transitions -m|--models <files|dirs>... [--alpha 1] -o <file.csv> <segment .csv | selection table>...\n" in err
    # the lines that were there stay as they were
    assert "                  --switch-penalty <x <= 0 | -inf> [-c <csv dir|file.csv>]\n                  [--posteriors [--frame-posteriors <dir>]]\n" in err
    assert "                  --posteriors adds each segment's mean and least class posterior, and the per-frame table)\n" in err


# ---- the report: CSV and stdout block of a hand-made segmentation ---------------------------------------------------------
def _report(tmp_path, capfd, cls, entered, ex, lp, ls, lt, names=("whale", "noise", "ship")):
    names_c, _k = hmm._strs(names)
    cls, entered, ex = np.array(cls, np.uint16), np.array(entered, np.uint8), np.array(ex, np.float64)
    lt = np.ascontiguousarray(lt, dtype=np.float64)
    csv = tmp_path / "rep" / "x.csv"
    capfd.readouterr()
    rc = e.lib.e2vq_hmm_segment_trans_report(b"x.wav", len(cls), len(names), names_c, 45, 15, cls.ctypes.data, entered.ctypes.data,
                                             ex.ctypes.data, lp, ls, lt.ctypes.data, str(csv).encode())
    assert rc == 0, _err()
    return csv.read_text().split("\n"), capfd.readouterr().out.split("\n")


def test_report_csv_and_block(tmp_path, capfd):
    g = lambda x: "%.17g" % x
    cls = [0, 0, 0, 1, 1, 1, 1, 1, 2, 2]
    entered = [1, 0, 0, 1, 0, 1, 0, 0, 1, 0]  # two adjacent segments of `noise`: [3, 5) and [5, 8)
    ex = [0.0, -1.0, -3.0, -6.0, -9.0, -13.5, -15.0, -19.0, -22.25, -26.0]
    lt = [[-9.0, -2.0, -9.0], [-9.0, -0.5, -4.0], [-9.0, -9.0, -9.0]]  # whale -> noise -2, noise -> noise -0.5, noise -> ship -4
    rows, out = _report(tmp_path, capfd, cls, entered, ex, -30.0, -1.0, lt)
    assert rows[0] == "segment,begin_frame,end_frame,begin_s,end_s,class,log_prob,log_prob_per_frame"
    assert rows[1] == f"0,0,3,0,{g(0.075)},whale,-6,-2"
    assert rows[2] == f"1,3,5,{g(0.045)},{g(0.105)},noise,-5.5,-2.75"            # -13.5 - (-6 - 2)
    assert rows[3] == f"2,5,8,{g(0.075)},{g(0.15)},noise,-8.25,-2.75"            # -22.25 - (-13.5 - 0.5)
    assert rows[4] == f"3,8,10,{g(0.12)},{g(0.18)},ship,-3.75,-1.875"            # -30 - (-22.25 - 4)
    assert rows[5] == "" and len(rows) == 6
    assert out[0] == "x.wav: T=10  segments=4  (switch penalty -1)"
    assert out[1:4] == ["  'whale': 3", "  'noise': 5", "  'ship': 2"]
    assert out[5:9] == ["    0.000 - 0.075 whale", "    0.045 - 0.105 noise", "    0.075 - 0.150 noise", "    0.120 - 0.180 ship"]
    assert out[9].endswith("x.csv saved")
    # the same arithmetic in the Python mirror and in the restatement
    segs = hmm.segments_of_trans(np.array(cls), np.array(entered), np.array(ex), -30.0, lt)
    want = [(0, 3, 0, -6.0), (3, 5, 1, -5.5), (5, 8, 1, -8.25), (8, 10, 2, -3.75)]
    assert [(s["begin"], s["end"], s["cls"], s["log_prob"]) for s in segs] == want
    assert RT.segments_of(cls, entered, ex, -30.0, lt) == want
    # with one price everywhere: the bytes of e2vq_hmm_segment_report
    rows_u, _out = _report(tmp_path, capfd, cls, entered, ex, -30.0, -2.0, np.full((3, 3), -2.0))
    names_c, _k = hmm._strs(("whale", "noise", "ship"))
    a, b, c = np.array(cls, np.uint16), np.array(entered, np.uint8), np.array(ex)
    assert e.lib.e2vq_hmm_segment_report(b"x.wav", 10, 3, names_c, 45, 15, a.ctypes.data, b.ctypes.data, c.ctypes.data, -30.0, -2.0,
                                         str(tmp_path / "plain.csv").encode()) == 0
    assert (tmp_path / "plain.csv").read_text().split("\n") == rows_u


def test_report_of_an_empty_stream_and_refusals(tmp_path, capfd):
    rows, out = _report(tmp_path, capfd, [], [], [], 0.0, -1.0, np.zeros((3, 3)))
    assert rows == ["segment,begin_frame,end_frame,begin_s,end_s,class,log_prob,log_prob_per_frame", ""]
    assert out[0] == "x.wav: T=0  segments=0  (switch penalty -1)"
    names_c, _k = hmm._strs(["a"])
    cls, entered, g = np.zeros(2, np.uint16), np.array([1, 0], np.uint8), np.zeros(2)
    rc = e.lib.e2vq_hmm_segment_trans_report(b"x", 2, 1, names_c, 45, 15, cls.ctypes.data, entered.ctypes.data, g.ctypes.data, -1.0, -1.0,
                                             None, str(tmp_path / "no.csv").encode())
    assert rc == 1 and "e2vq_hmm_segment_trans_report: bad arguments" in _err()
    assert not (tmp_path / "no.csv").exists()


# ---- the estimator ---------------------------------------------------------------------------------------------------------
def test_class_transitions_counts_bigrams_within_each_sequence():
    seqs = [[0, 1, 0, 1, 2], [2, 2], [1]]  # 0->1 x2, 1->0, 1->2, 2->2; no pair across two sequences
    c = np.array([[0, 2, 0], [1, 0, 1], [0, 0, 1]], dtype=np.float64)
    for alpha in (1.0, 0.25):
        lt = hmm.class_transitions(seqs, 3, alpha)
        want = [[math.log((c[f, k] + alpha) / (c[f].sum() + alpha * 3)) for k in range(3)] for f in range(3)]
        assert np.array_equal(_bits(lt), _bits(want))
    with np.errstate(divide="ignore"):
        lt = hmm.class_transitions(seqs, 3, 0.0)
    assert lt[0].tolist() == [NINF, 0.0, NINF] and lt[1].tolist() == [math.log(0.5), NINF, math.log(0.5)] and lt[2].tolist() == [NINF, NINF, 0.0]
    assert (lt <= 0.0).all()
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.class_transitions([[0, 1, 0]], 3, 0.0)
    assert "nothing follows class 2" in str(ei.value) and "alpha = 0" in str(ei.value)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.class_transitions([[0, 3]], 3)
    assert "label 3 at 1 is outside [0, 3)" in str(ei.value)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.class_transitions([[0, 1]], 2, -1.0)
    assert "alpha = -1" in str(ei.value)


def test_hmm_transitions_reads_segment_csvs_and_selection_tables(tmp_path):
    names = ["A", "B", "C"]
    for c in names:
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *_uniform(2, 4))
    # a segment CSV as e2vq_hmm_segment_report writes it: A B A C
    names_c, _k = hmm._strs(names)
    cls, entered = np.array([0, 0, 1, 0, 2, 2], np.uint16), np.array([1, 0, 1, 1, 1, 0], np.uint8)
    assert e.lib.e2vq_hmm_segment_report(b"x", 6, 3, names_c, 45, 15, cls.ctypes.data, entered.ctypes.data, np.zeros(6).ctypes.data, -1.0,
                                         -1.0, str(tmp_path / "seg.csv").encode()) == 0
    # a selection table: rows out of order, a comment, a label that is no model's class; by begin time: B A [?] B B
    (tmp_path / "sel.txt").write_text("# made by hand\nSelection\tBegin Time (s)\tEnd Time (s)\tType\n1\t2.5\t3.0\tA\n2\t0.5\t1.0\tB\n"
                                      "3\t4.0\t4.5\tmoan\n4\t7.25\t8.0\tB\n# a gap\n5\t5.0\t6.0\tB\n")
    rc, out, err = _cli(tmp_path, "transitions", "--models", "hmms", "--alpha", "0.5", "-o", "out/t.csv", "seg.csv", "sel.txt")
    assert rc == 0, (out, err)
    assert "2 inputs: 6 successions counted, 1 labels skipped" in out and "out/t.csv saved" in out
    # A->B, B->A, A->C | B->A, A->B, B->B
    lt = hmm.read_class_transitions(tmp_path / "out" / "t.csv", names)
    seqs = [[0, 1, 0, 2], [1, 0, 1, 1]]
    assert np.array_equal(_bits(lt), _bits(hmm.class_transitions(seqs, 3, 0.5)))
    hmm.class_transitions_files([str(tmp_path / "hmms" / f"{c}.hmm") for c in names], [str(tmp_path / "seg.csv"), str(tmp_path / "sel.txt")],
                                tmp_path / "py.csv", alpha=0.5)
    assert (tmp_path / "py.csv").read_bytes() == (tmp_path / "out" / "t.csv").read_bytes()
    # alpha = 0: nothing follows C
    rc, out, _err2 = _cli(tmp_path, "transitions", "--models", "hmms", "--alpha", "0", "-o", "out/t0.csv", "seg.csv", "sel.txt")
    assert rc == 1 and "nothing follows class 'C'" in out and not (tmp_path / "out" / "t0.csv").exists()
    (tmp_path / "other.csv").write_text("a,b\n1,2\n")
    rc, out, _err2 = _cli(tmp_path, "transitions", "--models", "hmms", "-o", "out/t1.csv", "other.csv")
    assert rc == 1 and "other.csv:1: neither a segment CSV" in out
    rc, _out, err = _cli(tmp_path, "transitions", "--models", "hmms", "seg.csv")
    assert rc == 2 and "hmm transitions: -o <file.csv> is required" in err


def test_library_exports():
    for name in ("e2vq_hmm_segment_trans", "e2vq_hmm_segment_trans_files", "e2vq_hmm_segment_trans_report",
                 "e2vq_hmm_segment_trans_last_kernel_ms", "e2vq_hmm_transitions_read", "e2vq_hmm_transitions_write",
                 "e2vq_hmm_class_transitions", "e2vq_hmm_transitions_files"):
        assert hasattr(e.lib, name)
    for fn in (hmm.segment_trans, hmm.segment_trans_last_kernel_ms, hmm.segments_of_trans, hmm.class_transitions,
               hmm.read_class_transitions, hmm.write_class_transitions, hmm.class_transitions_files):
        assert callable(fn)
    import inspect
    assert "class_transitions" in inspect.signature(hmm.segment_files).parameters


# ---- compiler metadata (read as test_hmm_segment_cpu.py reads its kernels') ---------------------------------------------------
VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_segment_trans.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_segment_trans.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _meta(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    return lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))


@pytest.mark.parametrize("pattern", [r"k_hmm_segment_transILb0ELb0E", r"k_hmm_segment_transILb0ELb1E", r"k_hmm_segment_transILb1ELb0E",
                                     r"k_hmm_segment_transILb1ELb1E", r"k_hmm_segment_trans_backtrackE"])
def test_trans_kernels_have_no_scratch_no_spill_and_fit_their_budget(asm, pattern):
    g = _meta(asm, pattern)
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
