"""`hmm align`, CPU side: the numpy restatement against a brute force over every admissible path, at L = 1
against the Viterbi restatement, and on the tie rules; on a planted stream, that the boundaries it finds are the planted ones;
the refusals of e2vq_hmm_align, e2vq_hmm_align_files and the CLI, which come before any HIP call; the label reader on both
formats; the exports, the Python surface and the usage text; the kernels' compiler metadata.  The GPU tests are in
test_gpu_hmm_align.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_align_cases as cases
from . import hmm_align_restatement as R
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


# ---- the restatement against a brute force over every admissible path ------------------------------------------------------------
BRUTE = [  # (N of the models, transcript, optional, T)
    ((2, 1), [0], [0], 1),
    ((2, 1), [0, 1], [0, 0], 2),
    ((2, 2), [0, 1, 0], [0, 1, 0], 5),
    ((2, 1, 2), [0, 0, 1, 2], [0, 0, 1, 0], 6),
    ((1, 2), [1, 0, 1, 1], [1, 0, 0, 1], 6),
    ((2, 2), [0, 1, 1, 0], [1, 0, 1, 0], 6),
    ((2, 2), [0, 1, 0, 1], [0, 0, 0, 0], 3),  # T < the mandatory units: status 1
]


@pytest.mark.parametrize("ls", [0.0, -1.5])
@pytest.mark.parametrize("case", range(len(BRUTE)))
def test_brute_force_over_every_admissible_path(case, ls):
    Ns, units, opt, T = BRUTE[case]
    for seed in range(6):
        rng = np.random.default_rng(100 * case + seed)
        models = [cases.random_model(rng, N, 3, zeros=0.4) for N in Ns]  # (zeros in pi and A: -inf occurs)
        lms = [V.log_model(*m) for m in models]
        seq = rng.integers(0, 3, T)
        got = R.align_logs(lms, seq, units, opt, ls)
        best, paths = R.brute_force(lms, seq, units, opt, ls)
        assert _bits(got["log_prob"]) == _bits(best), (seed, got["log_prob"], best)
        assert got["status"] == (1 if best == NINF else 0)
        if best != NINF:
            assert tuple(zip(got["unit"].tolist(), got["state"].tolist())) in paths, seed
            assert _bits(got["score"][-1]) == _bits(best)
            # entered marks exactly the frames where the unit changes, and begin / end are those frames
            u = got["unit"].astype(int)
            assert got["entered"].tolist() == [1] + [int(a != b) for a, b in zip(u[:-1], u[1:])]
            for l in range(len(units)):
                at = np.flatnonzero(u == l)
                assert (got["begin"][l], got["end"][l]) == ((at[0], at[-1] + 1) if len(at) else (-1, -1))
                assert len(at) or opt[l]
    if case == len(BRUTE) - 1:
        assert got["status"] == 1


@pytest.mark.parametrize("zeros", [0.0, 0.5])
def test_one_unit_is_the_viterbi_restatement(zeros):
    rng = np.random.default_rng(8)
    for N, T in ((1, 1), (5, 1), (5, 40), (64, 70)):
        model = cases.random_model(rng, N, cases.M, zeros)
        lm = V.log_model(*model)
        seq = rng.integers(0, cases.M, T)
        path, lp, status = V.viterbi_logs(*lm, seq)
        got = R.align_logs([lm], seq, [0], None, -2.0)
        assert np.array_equal(got["state"], path) and _bits(got["log_prob"]) == _bits(lp) and got["status"] == status
        assert got["unit"].tolist() == [0] * T and got["entered"].tolist() == [1] + [0] * (T - 1)
        assert (got["begin"][0], got["end"][0]) == (0, T)


# ---- ties ------------------------------------------------------------------------------------------------------------------------
def test_ties_stay_in_the_unit_leave_from_the_lowest_state_and_do_not_skip():
    # uniform models: every comparison of the recursion is a tie
    lms = [V.log_model(*_uniform(2, 4))] * 2
    # a duplicated class as neighbouring units: where staying ties with entering the back-pointer stays, so followed back from
    # the end the path is in the last unit for as long as that was alive: every unit is entered at the first frame it can be,
    # and left from its lowest state
    got = R.align_logs(lms, [0, 1, 2, 3, 0, 1], [0, 0, 1], None, 0.0)
    assert got["unit"].tolist() == [0, 1, 2, 2, 2, 2] and got["state"].tolist() == [0] * 6 and got["status"] == 0
    best, paths = R.brute_force(lms, [0, 1, 2, 3, 0, 1], [0, 0, 1], None, 0.0)
    assert _bits(best) == _bits(got["log_prob"]) and len(paths) > 1
    # an optional unit whose skip ties with its use: the last unit's model cannot emit symbol 1, so it is entered at frame 2 and
    # no sooner; at ln_switch = 0 unit 1, entered at frame 1, scores there what unit 0 scores, so unit 2 can be reached from
    # either at the same price: from the unit before, not over it
    tie_lms = [V.log_model(*m) for m in cases.skip_tie_models()]
    tie_seq, tie_units, tie_opt = cases.skip_tie()
    got = R.align_logs(tie_lms, tie_seq, tie_units, tie_opt, 0.0)
    assert got["unit"].tolist() == [0, 1, 2] and got["begin"].tolist() == [0, 1, 2] and got["end"].tolist() == [1, 2, 3]
    assert got["state"].tolist() == [0, 0, 0]
    _best, paths = R.brute_force(tie_lms, tie_seq, tie_units, tie_opt, 0.0)
    assert ((0, 0), (0, 0), (2, 0)) in paths  # (the skip reaches the same score)
    # where skipping is strictly better (the optional unit's model cannot emit the symbols) it is taken
    pi, A, B = _uniform(2, 4)
    dead = (pi, A, np.array([[0.0, 0.0, 0.0, 1.0]] * 2))
    got = R.align_logs([lms[0], V.log_model(*dead)], [0, 1, 2], [0, 1, 0], [0, 1, 0], 0.0)
    assert got["unit"].tolist() == [0, 2, 2] and got["begin"].tolist() == [0, -1, 1] and got["end"].tolist() == [1, -1, 3]


# ---- the planted stream ----------------------------------------------------------------------------------------------------------
# The restatement's worst boundary error on the three planted streams, at ln_switch = 0 and -3: 2 frames (fill "some"; 1 with
# "all", 0 with "none").  Allowed: that plus two frames.
PLANTED_TOLERANCE = 2 + 2


@pytest.mark.parametrize("ls", [0.0, -3.0])
@pytest.mark.parametrize("fill", ["all", "none", "some"])
def test_the_planted_boundaries_are_found(fill, ls):
    lms = [V.log_model(*m) for m in cases.planted_models()]
    sym, units, opt, truth = cases.planted(fill)
    got = R.align_logs(lms, sym, units, opt, ls)
    assert got["status"] == 0
    worst = 0
    for l in range(len(units)):
        if not opt[l]:
            assert got["begin"][l] >= 0
        if truth[l][0] >= 0 and got["begin"][l] >= 0:
            worst = max(worst, abs(int(got["begin"][l]) - int(truth[l][0])), abs(int(got["end"][l]) - int(truth[l][1])))
    print("worst boundary error", fill, ls, worst)
    assert worst <= PLANTED_TOLERANCE
    visited = got["begin"] >= 0
    if fill == "all":
        assert visited.all()  # skipping never wins
    if fill == "none" and ls == -3.0:
        assert not visited[opt != 0].any()  # skipping always wins


# ---- e2vq_hmm_align: refusals before the device ------------------------------------------------------------------------------------
def _align_c(models, sym, offs, units, unit_offs, optional=None, ls=-1.0, Ns=None, K=None, M=8):
    Ns = [len(m[0]) for m in models] if Ns is None else Ns
    K = len(models) if K is None else K
    n = max(len(models), 1)
    ns = (C.c_int * n)(*Ns)
    keep = [[np.ascontiguousarray(m[i], dtype=np.float64) for m in models] for i in range(3)]
    ptr = lambda i: (C.c_void_p * n)(*[a.ctypes.data for a in keep[i]])
    sym = np.ascontiguousarray(sym, dtype=np.uint16)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    units = np.ascontiguousarray(units, dtype=np.int32)
    unit_offs = np.ascontiguousarray(unit_offs, dtype=np.int64)
    opt = None if optional is None else np.ascontiguousarray(optional, dtype=np.uint8)
    return e.lib.e2vq_hmm_align(0, K, ns, M, ptr(0), ptr(1), ptr(2), sym.ctypes.data, offs.ctypes.data, len(offs) - 1, units.ctypes.data,
                                unit_offs.ctypes.data, None if opt is None else opt.ctypes.data, ls, None, None, None, None, None, None,
                                None, None, 0)


def _bad(where, value):
    pi, A, B = (x.copy() for x in _uniform(3, 8))
    {"pi": pi, "A": A, "B": B}[where].flat[1] = value
    return pi, A, B


@pytest.mark.parametrize("case,needle", [
    ("K0", "e2vq_hmm_align: 0 models (at least 1)"),
    ("N0", "e2vq_hmm_align: model 1 has N=0 states (1 .. 64)"),
    ("N65", "e2vq_hmm_align: model 0 has N=65 states (1 .. 64)"),
    ("sumN", "e2vq_hmm_align: 4160 states in all models (at most 4096)"),
    ("negative", "HMM parameter A[1] = -0.25: not a finite non-negative number"),
    ("nan", "HMM parameter pi[1] = nan: not a finite non-negative number"),
    ("offsets", "offs[2] = 40 < offs[1] = 50"),
    ("switch_nan", "e2vq_hmm_align: ln_switch = nan"),
    ("switch_pos", "e2vq_hmm_align: ln_switch = 0.5"),
    ("switch_ninf", "e2vq_hmm_align: ln_switch = -inf: a finite price"),
    ("empty", "e2vq_hmm_align: stream 1 has an empty transcript"),
    ("outside", "e2vq_hmm_align: stream 0, unit 2 names the class 2 outside [0, 2)"),
    ("negative_unit", "e2vq_hmm_align: stream 0, unit 0 names the class -1 outside [0, 2)"),
    ("adjacent", "e2vq_hmm_align: stream 0, units 1 and 2 are both optional"),
    ("all_optional", "e2vq_hmm_align: stream 0: every unit of the transcript is optional"),
    ("L", "e2vq_hmm_align: stream 0 has 65536 units (at most 65535)"),
    ("lds", "e2vq_hmm_align: stream 0: 20000 units of sum N = 60000 states do not fit in LDS"),
    ("lds_looped", "e2vq_hmm_align: stream 0: 3000 units of sum N = 9000 states in 143 wave-slots do not fit in LDS"),
    ("budget", "the back-pointers of 50 frames x (9 states + 3 units) take 600 bytes: more than ECOZ2_HMM_ALIGN_TABLE_BYTES=599"),
    ("body", "ECOZ2_HMM_ALIGN_BODY=fast: resident or looped"),
])
def test_align_refuses_before_the_device(case, needle, monkeypatch):
    ok = _uniform(3, 8)
    models, kw = [ok, ok], {}
    sym, offs, units, unit_offs, opt = np.zeros(50, np.uint16), [0, 50], [0, 1, 0], [0, 3], None
    if case == "K0":
        kw["K"] = 0
    elif case == "N0":
        kw["Ns"] = [3, 0]
    elif case == "N65":
        models = [_uniform(65, 8), ok]
    elif case == "sumN":
        models = [_uniform(64, 8)] * 65
    elif case == "negative":
        models = [ok, _bad("A", -0.25)]
    elif case == "nan":
        models = [_bad("pi", float("nan")), ok]
    elif case == "offsets":
        offs = [0, 50, 40]
        unit_offs = [0, 2, 3]
    elif case.startswith("switch"):
        kw["ls"] = {"switch_nan": float("nan"), "switch_pos": 0.5, "switch_ninf": NINF}[case]
    elif case == "empty":
        offs, unit_offs = [0, 20, 50], [0, 3, 3]
    elif case == "outside":
        units = [0, 1, 2]
    elif case == "negative_unit":
        units = [-1, 1, 0]
    elif case == "adjacent":
        opt = [0, 1, 1, 0]
        units, unit_offs = [0, 1, 0, 1], [0, 4]
    elif case == "all_optional":
        units, unit_offs, opt = [0], [0, 1], [1]
    elif case == "L":
        units, unit_offs = np.zeros(65536, np.int32), [0, 65536]
    elif case == "lds":
        units, unit_offs = np.zeros(20000, np.int32), [0, 20000]
    elif case == "lds_looped":
        units, unit_offs = np.zeros(3000, np.int32), [0, 3000]
    elif case == "budget":
        monkeypatch.setenv("ECOZ2_HMM_ALIGN_TABLE_BYTES", "599")
    else:
        monkeypatch.setenv("ECOZ2_HMM_ALIGN_BODY", "fast")
    assert _align_c(models, sym, offs, units, unit_offs, opt, **kw) == 1
    assert needle in _err(), _err()


def test_python_mirror_raises_the_refusal():
    ok = _uniform(3, 8)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.align([ok], np.zeros(4, np.uint16), [0, 4], [0, 0], [0, 2], optional=[1, 1])
    assert "every unit of the transcript is optional" in str(ei.value) or "both optional" in str(ei.value)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.align([ok], np.zeros(4, np.uint16), [0, 4], [0], [0, 1], ln_switch=1.0)
    assert "ln_switch = 1" in str(ei.value)
    with pytest.raises(ValueError):
        hmm.align([ok], np.zeros(4, np.uint16), [0, 4], [0], [0, 1, 1])
    with pytest.raises(ValueError):
        hmm.align_files(["a.hmm"], ["x.seq", "y.seq"], ["x.csv"])


def test_units_of_is_the_contracts_arithmetic():
    score = np.array([-1.0, -2.5, -4.0, -4.5, -7.0])
    got = hmm.units_of([2, 0, 1], [0, -1, 3], [3, -1, 5], score, -0.5)
    assert [(g["unit"], g["cls"], g["begin"], g["end"]) for g in got] == [(0, 2, 0, 3), (2, 1, 3, 5)]
    assert got[0]["score"] == -4.0 and got[1]["score"] == -7.0 - (-4.0 + -0.5)
    assert [tuple(g.values()) for g in got] == R.units_of([2, 0, 1], [0, -1, 3], [3, -1, 5], score, -0.5)


# ---- the label reader, e2vq_hmm_align_files and the CLI --------------------------------------------------------------------------
SEG_CSV = ("segment,begin_frame,end_frame,begin_s,end_s,class,log_prob,log_prob_per_frame\n"
           "0,0,10,0,0.18,A,-1,-0.1\n1,10,20,0.15,0.33,B,-1,-0.1\n2,20,40,0.3,0.63,B,-1,-0.1\n")
# rows out of order and comments: by begin time B A B B
SEL_TABLE = ("# made by hand\nSelection\tBegin Time (s)\tEnd Time (s)\tType\n1\t2.5\t3.0\tA\n2\t0.5\t1.0\tB\n"
             "4\t7.25\t8.0\tB\n# a gap\n5\t5.0\t6.0\tB\n")


@pytest.fixture
def corpus(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    for c, N in (("A", 3), ("B", 5), ("bg", 1)):
        hmm.save_model(d / f"{c}.hmm", c, *_uniform(N, 16))
    hmm.save_model(d / "C32.hmm", "C", *_uniform(3, 32))
    e.formats.write_seq(str(d / "x.seq"), "A", 16, np.arange(40) % 16)
    e.formats.write_prd(str(d / "x.prd"), "A", np.random.default_rng(1).uniform(0.1, 1.0, (40, 5)))
    (d / "seg.csv").write_text(SEG_CSV)
    (d / "sel.txt").write_text(SEL_TABLE)
    (d / "moan.txt").write_text(SEL_TABLE + "6\t0.25\t0.3\tmoan\n")
    (d / "moan.csv").write_text(SEG_CSV + "# a comment\n3,40,50,0.6,0.78,moan,-1,-0.1\n")
    (d / "empty.csv").write_text("class\n")
    (d / "other.csv").write_text("a,b\n1,2\n")
    return tmp_path, d, [str(d / "A.hmm"), str(d / "B.hmm"), str(d / "bg.hmm")]


def _align_files(models, inputs, labels, out, filler=None, codebook=None, ls=-1.0):
    m, _k1 = hmm._strs(models)
    f, _k2 = hmm._strs(inputs)
    l, _k3 = hmm._strs(labels)
    return e.lib.e2vq_hmm_align_files(m, len(models), str(codebook).encode() if codebook else None, f, l, len(inputs), 4, 45, 15, ls,
                                      filler, str(out).encode())


@pytest.mark.parametrize("labels,filler,units,states", [
    ("seg.csv", None, 3, 13),       # A B B
    ("sel.txt", None, 4, 18),       # B A B B
    ("seg.csv", b"bg", 7, 17),      # bg A bg B bg B bg
    ("sel.txt", b"bg", 9, 23),
])
def test_the_label_reader_gives_the_units_of_both_formats(corpus, labels, filler, units, states, monkeypatch):
    tmp_path, d, models = corpus
    # (a budget of one byte: the refusal names what the transcript came to, still before any HIP call)
    monkeypatch.setenv("ECOZ2_HMM_ALIGN_TABLE_BYTES", "1")
    assert _align_files(models, [str(d / "x.seq")], [str(d / labels)], tmp_path / "out", filler=filler) == 1
    assert f"{labels}: e2vq_hmm_align_files: stream 0: the back-pointers of 40 frames x ({states} states + {units} units)" in _err(), _err()
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("case,needle", [
    ("no_models", "e2vq_hmm_align_files: no models"),
    ("no_inputs", "e2vq_hmm_align_files: no inputs"),
    ("switch_pos", "e2vq_hmm_align_files: ln_switch = 2"),
    ("switch_ninf", "e2vq_hmm_align_files: ln_switch = -inf: a finite price"),
    ("models_M", "model has M=32 but"),
    ("filler", "e2vq_hmm_align_files: the filler 'wind' is no model's class"),
    ("foreign_table", "moan.txt:8: 'moan' is no model's class"),
    ("foreign_csv", "moan.csv:6: 'moan' is no model's class"),
    ("no_units", "empty.csv: no labelled units"),
    ("no_header", "other.csv:1: neither a segment CSV"),
    ("missing", "nowhere.csv"),
    ("no_codebook", "e2vq_hmm_align_files: signals and predictors need a codebook"),
    ("missing_input", "x.seq"),
])
def test_align_files_refuses_before_the_device(corpus, case, needle):
    tmp_path, d, models = corpus
    kw = {}
    inputs, labels = [str(d / "x.seq")], [str(d / "seg.csv")]
    if case == "no_models":
        models = []
    elif case == "no_inputs":
        inputs, labels = [], []
    elif case.startswith("switch"):
        kw["ls"] = 2.0 if case == "switch_pos" else NINF
    elif case == "models_M":
        models = models + [str(d / "C32.hmm")]
    elif case == "filler":
        kw["filler"] = b"wind"
    elif case == "foreign_table":
        labels = [str(d / "moan.txt")]
    elif case == "foreign_csv":
        labels = [str(d / "moan.csv")]
    elif case == "no_units":
        labels = [str(d / "empty.csv")]
    elif case == "no_header":
        labels = [str(d / "other.csv")]
    elif case == "missing":
        labels = [str(d / "nowhere.csv")]
    elif case == "no_codebook":
        inputs = [str(d / "x.prd")]
    else:
        inputs = [str(d / "nowhere" / "x.seq")]
    out = tmp_path / "out"
    assert _align_files(models, inputs, labels, out, **kw) == 1
    assert needle in _err(), _err()
    assert not out.exists()


def _cli(cwd, *args):
    r = subprocess.run([EXE, "hmm", *args], cwd=cwd, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("args,code,needle", [
    (["--labels", "in/seg.csv", "in/sel.txt"], 2, "hmm align: 2 label files for 1 inputs"),
    ([], 2, "hmm align: 0 label files for 1 inputs"),
    (["--labels", "in/seg.csv", "--switch-penalty", "1"], 2, "hmm align: --switch-penalty 1: finite and at most 0"),
    (["--labels", "in/seg.csv", "--switch-penalty", "-inf"], 2, "hmm align: --switch-penalty -inf: finite and at most 0"),
    (["--labels", "in/moan.txt"], 1, "in/moan.txt:8: 'moan' is no model's class"),
    (["--labels", "in/seg.csv", "--filler", "wind"], 1, "the filler 'wind' is no model's class"),
    (["--labels"], 2, "hmm align: 0 label files for 1 inputs"),
])
def test_cli_refusals(corpus, args, code, needle):
    tmp_path, _d, _models = corpus
    rc, out, err = _cli(tmp_path, "align", "--models", "in/A.hmm", "in/B.hmm", "in/bg.hmm", "--sequences", "in/x.seq", "-c", "out", *args)
    assert rc == code and needle in (err if code == 2 else out), (rc, out, err)
    assert not (tmp_path / "out").exists()


def test_usage_names_align_and_keeps_the_old_lines(tmp_path):
    rc, _out, err = _cli(tmp_path, "align")
    assert rc == 2
    assert "  ecoz2 hmm align -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15]\n" in err
    assert "[--switch-penalty <x <= 0>] [--filler <class>] [-c <csv dir|file.csv>] --labels <files>...\n" in err
    assert "  ecoz2 hmm segment -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15]\n" in err
    assert "                  --switch-penalty <x <= 0 | -inf> [-c <csv dir|file.csv>]\n" in err
    assert "                  [--continuous <name>]\n" in err
    assert "  ecoz2 hmm transitions -m|--models <files|dirs>... [--alpha 1] -o <file.csv> <segment .csv | selection table>...\n" in err
    assert "  ecoz2 hmm scan -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15] --window <frames>\n" in err
    assert "  ecoz2 hmm show --hmm <file> [-f|--format \"%Lg \"]\n" in err


def test_library_exports_and_python_surface():
    for name in ("e2vq_hmm_align", "e2vq_hmm_align_last_kernel_ms", "e2vq_hmm_align_report", "e2vq_hmm_align_files"):
        assert hasattr(e.lib, name)
    for name in ("align", "align_last_kernel_ms", "units_of", "align_files"):
        assert callable(getattr(hmm, name))


def test_report_csv_and_block(tmp_path, capfd):
    names_c, _k = hmm._strs(["A", "B", "bg"])
    units, opt = np.array([2, 0, 2, 1], np.int32), np.array([1, 0, 1, 0], np.uint8)
    begin, end = np.array([0, 2, -1, 5], np.int64), np.array([2, 5, -1, 8], np.int64)
    score = -np.arange(1.0, 9.0) * 1.25
    capfd.readouterr()
    assert e.lib.e2vq_hmm_align_report(b"x.seq", 8, 3, names_c, 45, 15, 4, units.ctypes.data, opt.ctypes.data, begin.ctypes.data,
                                       end.ctypes.data, score.ctypes.data, float(score[-1]), -0.5, str(tmp_path / "o" / "x.csv").encode()) == 0
    out = capfd.readouterr().out
    g = lambda v: "%.17g" % v
    want = "unit,class,begin_frame,end_frame,begin_s,end_s,score\n"
    for l, k, b, en, sc in R.units_of(units, begin, end, score, -0.5):
        want += f"{l},{['A', 'B', 'bg'][k]},{b},{en},{g(b * 15 / 1000.0)},{g(((en - 1) * 15 + 45) / 1000.0)},{g(sc)}\n"
    assert (tmp_path / "o" / "x.csv").read_text() == want and want.count("\n") == 4
    assert "x.seq: T=8  units=4  optional units passed over=1" in out and "(switch penalty -0.5)" in out
    assert "  'A': 3\n  'B': 3\n  'bg': 2\n" in out and "    0.030 - 0.105 A\n" in out and out.rstrip().endswith("x.csv saved")
    bad_end = np.array([2, 9, -1, 8], np.int64)
    assert e.lib.e2vq_hmm_align_report(b"x.seq", 8, 3, names_c, 45, 15, 4, units.ctypes.data, opt.ctypes.data, begin.ctypes.data,
                                       bad_end.ctypes.data, score.ctypes.data, 0.0, -0.5, None) == 1
    assert "e2vq_hmm_align_report: unit 1 spans [2, 9) of 8 frames" in _err()


# ---- the shapes where classes and units part: which instantiation each row of SHAPES reaches ---------------------------------------
def _header(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_restated_lds_constants_are_the_headers():
    dev = _header("hmm_device.h")
    lds = re.search(r"constexpr\s+size_t\s+SEG_LDS_BYTES\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", dev)
    waves = re.search(r"constexpr\s+int\s+SEG_MAX_WAVES\s*=\s*(\d+)\s*;", dev)
    assert lds and waves
    assert cases.SEG_LDS_BYTES == int(lds.group(1)) * int(lds.group(2)) and cases.SEG_MAX_WAVES == int(waves.group(1))
    pair = re.search(r"struct\s+Pair\s*\{[^\n]*\n(.*?)\};", _header("hmm_segment_common.h"), re.S)
    assert pair
    size = 0  # (a double and two ints: no padding between or behind them)
    for typ, names in re.findall(r"\b(double|int)\s+([^;]+);", pair.group(1)):
        size += {"double": 8, "int": 4}[typ] * len(names.split(","))
    assert cases.PAIR_BYTES == size == 16
    # the two sums themselves, term by term as the launchers write them
    align = re.search(r"size_t align_lds_bytes\([^)]*\)\s*\{(.*?)\n\}", _header("hmm_align.hip"), re.S).group(1)
    assert "SEG_MAX_WAVES * sizeof(Pair) + (size_t)2 * max_L * 8 + (a_lds ? (size_t)a_words * 8 : 0)" in align
    assert "(looped ? (size_t)2 * max_sumN * 8 : 0)" in align
    embed = re.search(r"size_t embed_lds_bytes\([^)]*\)\s*\{(.*?)\n\}", _header("hmm_embed.hip"), re.S).group(1)
    assert "(size_t)2 * SEG_MAX_WAVES * sizeof(double) + (size_t)2 * max_L * 8 + (a_lds ? (size_t)a_words * 8 : 0)" in embed
    assert "(an_lds ? (size_t)a_words * 16 : 0)" in embed


@pytest.mark.parametrize("name", list(cases.SHAPES))
def test_every_shape_reaches_the_instantiation_its_row_names(name):
    Ns, units, _opt, _T, _M, _zeros, _planted = cases.SHAPES[name]
    uN = [Ns[k] for k in units]
    L, sumN, a_words = len(uN), sum(uN), sum(N * N for N in Ns)
    looped, a_lds = cases.align_route(Ns, units)
    assert looped == (cases.slots_of(uN) > cases.SEG_MAX_WAVES)
    if name in cases.A_GLOBAL:  # lA overflows LDS under the body the row names, and the rest fits without it
        assert looped == (cases.A_GLOBAL[name] == "looped") and not a_lds
        assert cases.align_lds_bytes(L, sumN, a_words, looped, True) > cases.SEG_LDS_BYTES
        assert cases.align_lds_bytes(L, sumN, a_words, looped, False) <= cases.SEG_LDS_BYTES
        if not looped:  # (forced looped, the resident rows stay on global lA and still fit)
            assert cases.align_route(Ns, units, looped=True) == (True, False)
            assert cases.align_lds_bytes(L, sumN, a_words, True, False) <= cases.SEG_LDS_BYTES
    else:
        assert not looped and a_lds
    if looped:
        return  # (the E-step refuses more than 16 slots)
    e_words = sum(N * (N | 1) for N in Ns)
    if name in cases.A_GLOBAL:  # embed_plan chooses global A and global AN by itself
        assert cases.embed_route(Ns, L) == (False, False)
        assert cases.embed_lds_bytes(L, e_words, True, False) > cases.SEG_LDS_BYTES
        assert cases.embed_lds_bytes(L, e_words, False, True) > cases.SEG_LDS_BYTES
        assert cases.embed_lds_bytes(L, e_words, False, False) <= cases.SEG_LDS_BYTES
    else:
        assert cases.embed_route(Ns, L) == (True, True)


def test_the_shapes_are_what_their_rows_say():
    slots = {name: cases.slots_of([row[0][k] for k in row[1]]) for name, row in cases.SHAPES.items()}
    assert slots == {"64x6c_8u": 8, "64x6c_17u": 17, "21x48c": 16, "1x3c_200u": 4, "1x3c_201u_opt": 4, "1_64_1": 5, "mixed_M1024": 3,
                     "small_M65536": 1}
    units17 = cases.SHAPES["64x6c_17u"][1]
    assert len(units17) == 17 and sum(a == b for a, b in zip(units17, units17[1:])) == 1 and set(units17) == set(range(6))
    assert 200 % 64 == 8  # the last slot of "1x3c_200u" holds 8 lanes
    assert [m for _n, _u, _o, _t, m, _z, _p in cases.SHAPES.values()].count(8) == 6
    _models, _units, _opt, stream = cases.shape("small_M65536")
    assert stream[10] == stream[64] == 65535 and len(stream) == 70
    # every optional flag the batches carry is one align_plan accepts: no two in a row, never all
    for _models, _streams, transcripts, optionals in (cases.unlike_streams(), cases.random_batch(24, 40), cases.random_batch(24, 24, 16)):
        for u, o in zip(transcripts, optionals):
            assert len(u) == len(o) and not (o[1:] & o[:-1]).any() and not o.all()


# ---- compiler metadata (read as test_hmm_segment_stream_cpu.py reads its kernels') ------------------------------------------------
VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_align.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_align.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _meta(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    return lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))


@pytest.mark.parametrize("pattern", [r"k_hmm_alignILb0ELb0E", r"k_hmm_alignILb0ELb1E", r"k_hmm_alignILb1ELb0E", r"k_hmm_alignILb1ELb1E",
                                     r"k_hmm_align_backtrackE"])
def test_align_kernels_have_no_scratch_no_spill_and_fit_their_budget(asm, pattern):
    g = _meta(asm, pattern)
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
