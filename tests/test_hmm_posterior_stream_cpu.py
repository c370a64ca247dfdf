"""The posterior stream (`hmm segment --continuous-posteriors`), CPU side: the restatement's windowed rows
against an exact Fraction sum over every composite path of P(class at t | o[0 : w)); rows that sum to 1; the equality with the
closed restatement at L >= T; rows and ready counts that do not depend on how the stream was fed; the status rules; the
refusals of the entry points, the file form and the command line, which come before any HIP call; the usage text; and the
compiler's figures for the four kernel instantiations."""
import ctypes as C
import inspect
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_class_loop_cases as loop_cases
from . import hmm_posterior_restatement as R
from . import hmm_posterior_stream_restatement as RS
from .test_hmm_posteriors_cpu import _brute, _models, _uniform, tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXE = os.path.join(CSRC, "ecoz2")
NINF = float("-inf")
BODY = "ECOZ2_HMM_POSTERIOR_BODY"
SLOTS17 = "the classes take 17 wave-slots of 64 lanes (at most 16: the posteriors have no looped body)"


def _err():
    return e.lib.e2vq_last_error().decode()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@pytest.fixture(autouse=True)
def _no_body(monkeypatch):
    monkeypatch.delenv(BODY, raising=False)


# ---- the schedule -------------------------------------------------------------------------------------------------------------
def test_ready_after_counts_the_blocks_whose_window_has_been_fed():
    for B, L in ((1, 0), (1, 3), (4, 0), (4, 3), (4, 4), (64, 100)):
        s = RS.Stream([_uniform(2, 3)], -1.0, B, L)
        for p in range(0, 3 * (B + L) + 2):
            want = sum(B for b in range(p + 1) if s.window_end(b) <= p)
            assert s.ready_after(p) == want == RS.ready_after(p, B, L), (B, L, p)
    assert RS.Stream([_uniform(2, 3)], -1.0, 4, 3).window_end(2) == 15


# ---- the windowed rows are P(class at t | the first w symbols) -------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "uniform"])
@pytest.mark.parametrize("Ns", [(1,), (2, 1), (1, 1, 2)])
def test_windowed_rows_against_every_composite_path(kind, Ns):
    M, T = 3, 7
    models = _models(kind, Ns, M, 5)
    seq = np.random.default_rng(sum(Ns)).integers(0, M, T)
    brute = {}
    worst = 0.0
    for ls in (NINF, -3.0, 0.0):
        for B, L in ((1, 0), (2, 1), (3, 2), (2, 5), (4, 0)):
            s, _ready, rows = RS.run(models, seq, ls, B, L, [T])
            assert s.status == 0 and rows.shape == (T, len(Ns))
            for t in range(T):
                w = min(s.window_end(t // B), T)
                if (ls, w) not in brute:
                    brute[ls, w] = _brute(models, seq[:w], ls)[0]
                tol = tolerance(w, max(Ns))  # (4.8.7's formula with T taken as w)
                for k in range(len(Ns)):
                    err = abs(float(Fraction(float(rows[t, k])) - brute[ls, w][t][k]))
                    worst = max(worst, err / tol)
                    assert err <= tol, (ls, B, L, t, k, w, err, tol)
                assert abs(float(np.sum(rows[t])) - 1.0) <= tol, (ls, B, L, t)
    print(f"worst error / tolerance: {worst:.4f}")


def _clean(T, seed=130):
    return np.random.default_rng(seed).integers(0, loop_cases.DEAD, T).astype(np.uint16)


@pytest.mark.parametrize("B,L", [(1, 0), (5, 0), (5, 3), (8, 8), (64, 100)])
def test_rows_sum_to_one(B, L):
    models, seq = loop_cases.event_models(), _clean(40)
    s, _ready, rows = RS.run(models, seq, -0.5, B, L, [len(seq)])
    for t in range(len(seq)):
        w = min(s.window_end(t // B), len(seq))
        assert abs(float(np.sum(rows[t])) - 1.0) <= tolerance(w, 5), (t, w)


# ---- L >= T: the closed pass --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0, 1, 9, 40])
def test_a_look_ahead_of_the_whole_stream_gives_the_closed_pass(T):
    models, seq = loop_cases.event_models(), _clean(T)
    want = R.posteriors_one(models, seq, -0.5)
    for B, L in ((1, T), (7, T), (7, T + 5), (64, 64)):
        s, ready, rows = RS.run(models, seq, -0.5, B, L, [T])
        assert ready == [0] and s.ready == T and s.status == 0
        assert np.array_equal(_bits(rows), _bits(want["post"])) and _bits(s.log_prob) == _bits(want["log_prob"])
    # and every block whose window reaches the end of the stream
    s, _ready, rows = RS.run(models, seq, -0.5, 4, 6, [T])
    for t in range(T):
        if s.window_end(t // 4) >= T:
            assert np.array_equal(_bits(rows[t]), _bits(want["post"][t]))
    assert _bits(s.log_prob) == _bits(want["log_prob"])


def test_nothing_fed():
    s = RS.Stream(loop_cases.event_models(), -0.5, 4, 2)
    assert s.feed([]) == (0, pytest.approx(np.zeros((0, 3))))
    first, rows = s.close()
    assert (first, rows.shape, s.status, s.log_prob, s.launches) == (0, (0, 3), 0, 0.0, 0)


# ---- however it was fed -----------------------------------------------------------------------------------------------------------
def _feeds(T, sizes):
    out = []
    while sum(out) < T:
        out.append(min(sizes[len(out) % len(sizes)], T - sum(out)))
    return out


@pytest.mark.parametrize("B,L", [(5, 0), (5, 3), (8, 8), (3, 11)])
def test_three_feed_patterns_give_the_same_rows_and_ready_counts(B, L):
    models, seq = loop_cases.event_models(), _clean(61)
    T = len(seq)
    cache = {}
    whole, _r, rows = RS.run(models, seq, -0.5, B, L, [T], cache=cache)
    for feeds in (_feeds(T, (B,)), _feeds(T, (B - 1, B, B + 1)), [1] * T):
        s = RS.Stream(models, -0.5, B, L, cache=cache)
        at, got = 0, []
        for n in feeds:
            first, part = s.feed(seq[at:at + n])
            at += n
            assert s.ready == s.ready_after(at) and first + len(part) == s.ready
            got.extend(part)
        first, part = s.close()
        got.extend(part)
        assert s.ready == T and np.array_equal(_bits(np.array(got)), _bits(rows))
        assert (s.launches, s.walked, _bits(s.log_prob)) == (whole.launches, whole.walked, _bits(whole.log_prob))
    # the forward pass sees every frame once; the backward pass of a window walks B + L frames
    full = (T - L) // B
    assert whole.launches == full + 1 and whole.walked == full * (B + L) + (T - full * B)


# ---- status -----------------------------------------------------------------------------------------------------------------------
B_EV, L_EV, T_EV = 8, 5, 40  # windows end at 13, 21, 29, 37; close serves [32, 40)


def _event_stream(at, symbol):
    seq = _clean(T_EV)
    seq[at] = symbol
    return seq


@pytest.mark.parametrize("at", [0, 7, 8, 12, 13, 20, 36, 37, 39])
@pytest.mark.parametrize("kind", ["M", "dead"])
def test_the_first_event_decides(kind, at):
    models = loop_cases.event_models()
    seq = _event_stream(at, loop_cases.EVENT_M if kind == "M" else loop_cases.DEAD)
    s = RS.Stream(models, -0.5, B_EV, L_EV)
    clean, _r, clean_rows = RS.run(models, _clean(T_EV), -0.5, B_EV, L_EV, [T_EV])
    delivered = RS.ready_after(at, B_EV, L_EV)  # the windows that ended at or before the event
    fed, raised = 0, None
    for n in _feeds(T_EV, (7, 9)):
        try:
            s.feed(seq[fed:fed + n])
        except RS.BadSymbol as ex:
            raised = ex.frame
        fed += n
        if raised is not None:
            break
        assert s.ready == min(s.ready_after(fed), delivered)
    if kind == "M":
        met_by_feed = at < RS.ready_after(T_EV, B_EV, L_EV) + L_EV  # (below the last window end a feed reaches)
        assert (raised == at) == met_by_feed
        if raised is not None:
            with pytest.raises(RS.Refused):
                s.feed(seq[fed:])
            first, rows = s.close()
        else:
            with pytest.raises(RS.BadSymbol) as ei:
                s.close()
            assert ei.value.frame == at
            first, rows = s.take()
    else:
        assert raised is None and fed == T_EV
        first, rows = s.close()
    assert s.status == (2 if kind == "M" else 1) and s.frame == at and s.log_prob == NINF and s.ready == s.fed
    every = np.array(s.rows)
    assert np.array_equal(_bits(every[:delivered]), _bits(clean_rows[:delivered]))
    assert not every[delivered:].any() and not np.signbit(every[delivered:]).any() and len(every) == s.fed
    with pytest.raises(RS.Refused):
        s.close()


def test_a_bad_symbol_comes_before_the_arithmetic_of_its_frame_and_the_earlier_event_wins():
    models = loop_cases.event_models()
    seq = _clean(T_EV)
    seq[9], seq[10] = loop_cases.DEAD, loop_cases.EVENT_M
    s = RS.run(models, seq, -0.5, B_EV, L_EV, [T_EV])[0]
    assert (s.status, s.frame) == (1, 9)
    seq[9], seq[10] = loop_cases.EVENT_M, loop_cases.DEAD
    s = RS.Stream(models, -0.5, B_EV, L_EV)
    with pytest.raises(RS.BadSymbol):
        s.feed(seq)
    assert (s.status, s.frame, s.ready) == (2, 9, 0)


# ---- refusals before any HIP call ---------------------------------------------------------------------------------------------------
def _open_c(models, ln_switch, block=4, lookahead=2, Ns=None, K=None, out=True):
    Ns = [len(m[0]) for m in models] if Ns is None else Ns
    K = len(models) if K is None else K
    n = max(len(models), 1)
    ns = (C.c_int * n)(*Ns)
    keep = [[np.ascontiguousarray(m[i], dtype=np.float64) for m in models] for i in range(3)]
    ptr = lambda i: (C.c_void_p * n)(*[a.ctypes.data for a in keep[i]])
    h = C.c_void_p()
    rc = e.lib.e2vq_hmm_posterior_stream_open(0, K, ns, 8, ptr(0), ptr(1), ptr(2), ln_switch, block, lookahead,
                                              C.byref(h) if out else None)
    if h:
        e.lib.e2vq_hmm_posterior_stream_free(h)
    return rc


def _bad(where, value):
    pi, A, B = (x.copy() for x in _uniform(3, 8))
    {"pi": pi, "A": A, "B": B}[where].flat[1] = value
    return pi, A, B


WHO = "e2vq_hmm_posterior_stream_open: "


@pytest.mark.parametrize("case,needle", [
    ("K0", WHO + "0 models (at least 1)"),
    ("no_out", WHO + "bad arguments"),
    ("N65", WHO + "model 0 has N=65 states (1 .. 64)"),
    ("sumN", WHO + "4160 states in all models (at most 4096)"),
    ("negative", "HMM parameter A[1] = -0.25: not a finite non-negative number"),
    ("nan", "HMM parameter pi[1] = nan: not a finite non-negative number"),
    ("switch_nan", WHO + "ln_switch = nan"),
    ("switch_pos", WHO + "ln_switch = 0.5"),
    ("slots17", WHO + SLOTS17),
    ("block0", WHO + "a block of 0 frames (at least 1)"),
    ("block_neg", WHO + "a block of -4 frames (at least 1)"),
    ("look_neg", WHO + "a look-ahead of -1 frames (at least 0)"),
])
def test_open_refuses_before_the_device(case, needle):
    ok = _uniform(3, 8)
    rc = {
        "K0": lambda: _open_c([ok], -1.0, K=0),
        "no_out": lambda: _open_c([ok], -1.0, out=False),
        "N65": lambda: _open_c([_uniform(65, 8)], -1.0),
        "sumN": lambda: _open_c([_uniform(64, 8)] * 65, -1.0),
        "negative": lambda: _open_c([ok, _bad("A", -0.25)], -1.0),
        "nan": lambda: _open_c([_bad("pi", float("nan"))], -1.0),
        "switch_nan": lambda: _open_c([ok], float("nan")),
        "switch_pos": lambda: _open_c([ok], 0.5),
        "slots17": lambda: _open_c([_uniform(64, 8)] * 17, -1.0),
        "block0": lambda: _open_c([ok], -1.0, block=0),
        "block_neg": lambda: _open_c([ok], -1.0, block=-4),
        "look_neg": lambda: _open_c([ok], -1.0, lookahead=-1),
    }[case]()
    assert rc == 1 and (_err().startswith(needle) if needle.startswith(WHO) else needle in _err()), _err()


def test_the_body_variable_is_read_at_open(monkeypatch):
    wide = [_uniform(64, 8)] * 17
    monkeypatch.setenv(BODY, "fast")
    assert _open_c([_uniform(3, 8)], -1.0) == 1 and _err() == BODY + "=fast: auto, resident or looped"
    monkeypatch.setenv(BODY, "resident")
    assert _open_c(wide, -1.0) == 1 and _err() == WHO + SLOTS17
    for body in ("auto", "looped"):  # as far as the device
        monkeypatch.setenv(BODY, body)
        rc = _open_c(wide, -1.0)
        assert rc == 0 if e.lib.e2vq_device_count() > 0 else (rc == 1 and "no HIP device" in _err()), _err()
    # the block and the look-ahead are held against their bounds before the device is asked for
    assert _open_c(wide, -1.0, block=0) == 1 and "a block of 0 frames" in _err()


def test_null_sessions_are_refused():
    n = C.c_int64()
    assert e.lib.e2vq_hmm_posterior_stream_feed(None, None, 0, 0, C.byref(n)) == 1 and "e2vq_hmm_posterior_stream_feed: NULL session" in _err()
    assert e.lib.e2vq_hmm_posterior_stream_close(None, None, None, None) == 1 and "e2vq_hmm_posterior_stream_close: NULL session" in _err()
    assert e.lib.e2vq_hmm_posterior_stream_take(None, 0, None, None, None) == 1 and "NULL session" in _err()
    assert e.lib.e2vq_hmm_posterior_stream_kernel_ms(None, None) == 1 and "NULL session" in _err()
    assert e.lib.e2vq_hmm_posterior_stream_stats(None, None, None, None, None) == 1 and "NULL session" in _err()
    e.lib.e2vq_hmm_posterior_stream_free(None)


def test_python_mirror():
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.PosteriorStream([_uniform(3, 8)], -1.0, block=0)
    assert "a block of 0 frames" in str(ei.value)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.PosteriorStream([_uniform(64, 8)] * 17, -1.0)
    assert SLOTS17 in str(ei.value) and BODY not in os.environ
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.PosteriorStream([_uniform(3, 8)], -1.0, body="fast")
    assert BODY + "=fast" in str(ei.value) and BODY not in os.environ
    params = inspect.signature(hmm.PosteriorStream.__init__).parameters
    assert [params[k].default for k in ("block", "lookahead", "device", "body")] == [4096, 4096, 0, None]
    params = inspect.signature(hmm.segment_files).parameters
    assert list(params)[-3:] == ["continuous_posteriors", "block", "lookahead"]
    assert [params[k].default for k in list(params)[-3:]] == [None, 4096, 4096]
    for other in (dict(continuous="r"), dict(posteriors=True), dict(class_transitions="t.csv"), dict(grammar_continuous="r"),
                  dict(grammar_body="auto"), dict(grammar_posteriors_body="auto"), dict(grammar_posteriors=True)):
        with pytest.raises(ValueError):
            hmm.segment_files(["a.hmm"], ["x.seq"], -1.0, continuous_posteriors="rec", **other)


def test_files_refuse_before_the_device(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    many = []
    for k in range(17):
        hmm.save_model(d / f"c{k:02d}.hmm", f"c{k:02d}", *_uniform(64, 16))
        many.append(str(d / f"c{k:02d}.hmm"))
    e.formats.write_seq(str(d / "x.seq"), "A", 16, np.arange(40) % 16)
    e.formats.write_seq(str(d / "y.seq"), "A", 32, np.arange(40) % 32)
    who = "e2vq_hmm_segment_continuous_files_posteriors: "

    def files(models, inputs, ls=-5.0, name="rec", csv=None, frames=None, block=8, lookahead=8):
        m, _k1 = hmm._strs(models)
        f, _k2 = hmm._strs(inputs)
        return e.lib.e2vq_hmm_segment_continuous_files_posteriors(
            m, len(models), None, f, len(inputs), 4, 45, 15, ls, name.encode() if name is not None else None,
            str(csv).encode() if csv else None, str(frames).encode() if frames else None, block, lookahead)

    out = tmp_path / "out"
    x = [str(d / "x.seq")]
    assert files([], x, csv=out) == 1 and _err() == who + "no models"
    assert files(many[:2], [], csv=out) == 1 and _err() == who + "no inputs"
    assert files(many[:2], x, name="", csv=out) == 1 and _err() == who + "the recording needs a name"
    assert files(many[:2], x, ls=2.0, csv=out) == 1 and _err().startswith(who + "ln_switch = 2")
    assert files(many, x, csv=out, frames=out) == 1 and _err() == who + SLOTS17
    assert files(many[:2], x, csv=out, block=0) == 1 and _err() == who + "a block of 0 frames (at least 1)"
    assert files(many[:2], x, csv=out, lookahead=-3) == 1 and _err() == who + "a look-ahead of -3 frames (at least 0)"
    assert files(many[:2], [str(d / "y.seq")], csv=out) == 1 and "codebook size 32 differs from the models' 16" in _err(), _err()
    assert not out.exists()
    rc = files(many[:2], x)
    assert rc == 0 if e.lib.e2vq_device_count() > 0 else (rc == 1 and "no HIP device" in _err()), _err()


# ---- the command line -------------------------------------------------------------------------------------------------------------
def _cli(cwd, *args):
    r = subprocess.run([EXE, "hmm", "segment", *args], cwd=cwd, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


BASE = ("--models", "a.hmm", "--sequences", "x.seq", "--switch-penalty", "-5")
NOT_WITH = ("hmm segment: --continuous-posteriors gives the posteriors of one stream under the one switch penalty: not with --continuous, "
            "--posteriors, --class-transitions, --grammar-posteriors, --grammar-continuous, --grammar-body or --grammar-posteriors-body\n")


@pytest.mark.parametrize("other", [("--continuous", "r"), ("--posteriors",), ("--class-transitions", "t.csv"), ("--grammar-posteriors",),
                                   ("--grammar-continuous", "r"), ("--grammar-body", "auto"), ("--grammar-posteriors-body", "auto")])
def test_cli_refuses_the_flag_next_to_another_mode(tmp_path, other):
    rc, out, err = _cli(tmp_path, *BASE, "--continuous-posteriors", "rec", *other)
    assert (rc, out, err) == (2, "", NOT_WITH)


def test_cli_refusals_of_its_own_values(tmp_path):
    needs = "hmm segment: --block and --lookahead need --continuous-posteriors <name> (they are its block and its look-ahead)\n"
    assert _cli(tmp_path, *BASE, "--block", "64") == (2, "", needs)
    assert _cli(tmp_path, *BASE, "--lookahead", "64", "--posteriors") == (2, "", needs)
    assert _cli(tmp_path, *BASE, "--continuous-posteriors", "rec", "--block", "0") == (2, "", "hmm segment: --block 0: at least 1 frame\n")
    assert _cli(tmp_path, *BASE, "--continuous-posteriors", "rec", "--lookahead", "-1") == (2, "", "hmm segment: --lookahead -1: at least 0 frames\n")
    assert _cli(tmp_path, *BASE, "--continuous-posteriors", "") == (2, "", "hmm segment: --continuous-posteriors <name>: the recording needs a name\n")
    assert _cli(tmp_path, *BASE, "--continuous-posteriors") == (2, "", "--continuous-posteriors needs a value\n")
    assert _cli(tmp_path, *BASE, "--continuous-posteriors", "rec", "--block", "x")[2] == "--block: invalid value 'x'\n"
    rc, _out, err = _cli(tmp_path, *BASE, "--continuous-posteriors", "rec", "--body", "fast")
    assert rc == 2 and "hmm segment --continuous-posteriors: --body fast" in err
    # what stood before still stands
    rc, _out, err = _cli(tmp_path, *BASE, "--continuous", "r", "--posteriors")
    assert rc == 2 and err == "hmm segment: --continuous decodes under the one switch penalty: not with --posteriors or --class-transitions\n"
    rc, _out, err = _cli(tmp_path, *BASE, "--frame-posteriors", "frames")
    assert rc == 2 and err == "hmm segment: --frame-posteriors <dir> needs --posteriors\n"
    rc, _out, err = _cli(tmp_path, *BASE, "--body", "auto")
    assert rc == 2 and err == "hmm segment: --body <auto|resident|looped> needs --posteriors\n"
    assert not any(tmp_path.iterdir())


def test_usage_has_a_block_of_its_own_between_the_grammar_session_and_the_transitions(tmp_path):
    rc, _out, err = _cli(tmp_path)
    assert rc == 2
    new = ("                  --switch-penalty <x <= 0 | -inf> --continuous-posteriors <name> [--block 4096] [--lookahead 4096]\n"
           "                  [--frame-posteriors <dir>] [--body <auto|resident|looped>] [-c <csv dir|file.csv>]\n")
    assert err.count(new) == 1 and err.count("--continuous-posteriors") == 2
    at = err.index(new)
    assert err.index("under the prices of --class-transitions)\n") < at < err.index("  ecoz2 hmm transitions -m|--models")
    # the text without the new block is the text of the lines that stood before, in their order
    lines = err.splitlines(keepends=True)
    first = next(i for i, l in enumerate(lines) if "--continuous-posteriors <name> [--block" in l) - 1
    assert lines[first].startswith("  ecoz2 hmm segment -m|--models") and lines[first + 8].startswith("  ecoz2 hmm transitions -m|--models")
    old = "".join(lines[:first] + lines[first + 8:])
    assert "--continuous-posteriors" not in old and "--lookahead" not in old
    for line in ("                  [--grammar-posteriors [--frame-posteriors <dir>]]\n", "                  [--continuous <name>]\n",
                 "                  --switch-penalty <x <= 0 | -inf> --class-transitions <file.csv> --grammar-continuous <name>\n",
                 "                  (--continuous <name>: the inputs are consecutive pieces of one recording, decoded as one stream)\n"):
        assert old.count(line) == 1


def test_library_exports_and_header():
    names = ["e2vq_hmm_posterior_stream_" + n for n in ("open", "feed", "close", "take", "kernel_ms", "stats", "free")]
    names.append("e2vq_hmm_segment_continuous_files_posteriors")
    header = open(os.path.join(ROOT, "include", "ecoz2_classify.h")).read()
    for name in names:
        assert isinstance(getattr(e.lib, name), C._CFuncPtr) and name + "(" in header
    assert "typedef struct e2vq_posterior_stream e2vq_posterior_stream;" in header
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert " hmm_posterior_stream_dev.o hmm_posterior_stream.o " in mk and " hmm_posterior_stream.h " in mk
    host = open(os.path.join(CSRC, "hmm_posterior_stream.cpp")).read()
    for shared in ("pack_slots(", "ClassLoopDev loop", "posteriors_body(", "posteriors_check_slots(", "SymStage stg", "sym_inputs_check(",
                   "embed_params(", "e2vq_hmm_segment_report_posteriors("):
        assert shared in host, shared


# ---- compiler metadata (read as test_hmm_posteriors_looped_cpu.py reads its kernels') -----------------------------------------------
VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_posterior_stream.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_posterior_stream.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _meta(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    return lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))


@pytest.mark.parametrize("pattern", [r"k_hmm_loop_posteriors_streamILb0EE", r"k_hmm_loop_posteriors_streamILb1EE",
                                     r"k_hmm_loop_posteriors_stream_loopedILb0EE", r"k_hmm_loop_posteriors_stream_loopedILb1EE"])
def test_stream_kernels_have_no_scratch_no_spill_and_fit_their_budget(asm, pattern):
    g = _meta(asm, pattern)
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    # (all LDS is dynamic: its base stays 16-byte aligned)
    assert set(re.findall(r"\.group_segment_fixed_size:\s+(\d+)", asm)) == {"0"}
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
    assert "buffer_store" not in asm and "scratch_" not in asm


def test_the_kernels_take_their_helpers_from_the_lane_header():
    src = open(os.path.join(CSRC, "hmm_posterior_stream.hip")).read()
    assert '#include "hmm_lane.h"' in src and "asm(" not in src and "asm volatile" not in src
    for fn in ("chain_col(", "chain_row(", "chain_sum(", "block_sum(", "slot_sum(", "slots_sum(", "scale_step("):
        assert fn in src and "double " + fn not in src and "void " + fn not in src, fn
