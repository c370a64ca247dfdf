"""`hmm segment --posteriors`, CPU side: the numpy restatement against the contract transcribed in plain
loops, against an exact Fraction sum over every composite path and against an np.longdouble forward-backward written
independently; the rows of post summing to 1; the argument checks of e2vq_hmm_segment_posteriors and of the file form, which
run before any HIP call; the CSV columns, the p= field and the per-frame table of e2vq_hmm_segment_report_posteriors on
hand-made arrays; the exports and the usage text; the kernel's compiler metadata.  The GPU parity tests are in
test_gpu_hmm_posteriors.py."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_posterior_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXE = os.path.join(CSRC, "ecoz2")
NINF = float("-inf")
U = 2.0 ** -53


def _err():
    return e.lib.e2vq_last_error().decode()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _uniform(N, M):
    return np.full(N, 1.0 / N), np.full((N, N), 1.0 / N), np.full((N, M), 1.0 / M)


def _random(rng, N, M):
    rows = lambda n, m: (lambda x: x / x.sum(axis=1, keepdims=True))(rng.uniform(0.05, 1.0, (n, m)))
    return rows(1, N)[0], rows(N, N), rows(N, M)


def _models(kind, Ns, M, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return [_random(rng, N, M) for N in Ns]
    if kind == "uniform":
        return [_uniform(N, M) for N in Ns]
    hmm.set_random_seed(seed)
    return [hmm.init_model(N, M, 2 if kind == "cascade2" else 3) for N in Ns]


def tolerance(T, Nmax):
    """first order, every term non-negative, so relative errors add: per step at most N + 1 roundings in the chain, the enter
    add, the emission product, <= 22 in the global sum and one division -- N + 32 bounds them; 2 T + 1 steps lie between a
    posterior and the parameters (T forward, T backward, the product and the class sum); the factor 4 covers the second
    order.  A posterior is at most 1, so the relative bound is an absolute one."""
    return 4.0 * (2 * T + 1) * (Nmax + 32) * U


# ---- restatement == transcription ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "uniform", "cascade2", "cascade3"])
@pytest.mark.parametrize("Ns", [(1,), (3,), (1, 1), (2, 3, 3, 1), (30, 30, 30), (64, 5)])
def test_restatement_equals_the_transcription(kind, Ns):
    M = 5
    models = _models(kind, Ns, M, 11)
    rng = np.random.default_rng(len(Ns))
    for T in (0, 1, 2, 7, 12 if max(Ns) > 8 else 40):
        seq = rng.integers(0, M, T)
        for ls in (NINF, -20.0, -3.0, 0.0):
            got = R.posteriors_one(models, seq, ls)
            post, lp, st = R.transcribe(models, seq, ls)
            assert got["status"] == st and _bits(got["log_prob"]) == _bits(lp)
            assert got["post"].shape == (T, len(Ns)) and np.array_equal(_bits(got["post"]), _bits(np.array(post).reshape(T, len(Ns))))
    got = R.posteriors_one(models, [1, M, 2], -1.0)
    assert (got["post"].tolist(), got["log_prob"], got["status"]) == R.transcribe(models, [1, M, 2], -1.0)
    assert got["status"] == 2 and got["log_prob"] == NINF and not got["post"].any()


def test_packing_and_the_empty_stream():
    slot, lane, slots = R.packing([5] * 13)
    assert slots == 2 and slot.tolist() == [0] * 60 + [1] * 5 and lane.tolist() == list(range(60)) + list(range(5))
    slot, lane, slots = R.packing([21, 22, 64])
    assert slots == 2 and lane[:43].tolist() == list(range(43)) and lane[43:].tolist() == list(range(64))
    assert R.packing([64] * 17)[2] == 17
    got = R.posteriors_one([_uniform(2, 3)], [], -1.0)
    assert got["post"].shape == (0, 1) and got["log_prob"] == 0.0 and got["status"] == 0
    assert R.log_prob(0.5, 1) == 0.0


# ---- brute force: an exact sum over every composite path ------------------------------------------------------------------
def _brute(models, seq, ls):
    """exact post (T x K Fractions) and P(O | loop): the sum over every path of composite states of pi B prod (W B), where
    one step from (k, i) to (k', j) weighs [k == k'] A_k[i][j] (a stay) + sw pi_k'[j] (an entry; the same class included)"""
    F = lambda x: Fraction(float(x))
    sw = F(math.exp(ls))
    states = [(k, j) for k, m in enumerate(models) for j in range(len(m[0]))]
    K, T = len(models), len(seq)
    num = [[Fraction(0)] * K for _ in range(T)]
    total = Fraction(0)
    for path in itertools.product(states, repeat=T):
        k, j = path[0]
        w = F(models[k][0][j]) * F(models[k][2][j][seq[0]])
        for t in range(1, T):
            k2, j2 = path[t]
            step = sw * F(models[k2][0][j2])
            if k2 == k:
                step += F(models[k][1][j][j2])
            w *= step * F(models[k2][2][j2][seq[t]])
            k, j = k2, j2
        total += w
        for t in range(T):
            num[t][path[t][0]] += w
    return [[x / total for x in row] for row in num], total


@pytest.mark.parametrize("kind", ["random", "uniform"])
@pytest.mark.parametrize("Ns", [(1,), (2, 1), (2, 3), (1, 1, 2)])
def test_brute_force_over_every_composite_path(kind, Ns):
    M = 3
    models = _models(kind, Ns, M, 5)
    rng = np.random.default_rng(sum(Ns))
    worst = 0.0
    for T in (1, 2, 3, 4, 5):
        seq = rng.integers(0, M, T)
        tol = tolerance(T, max(Ns))
        for ls in (NINF, -3.0, 0.0):
            r = R.posteriors_one(models, seq, ls)
            want, total = _brute(models, seq, ls)
            assert r["status"] == 0
            for t in range(T):
                for k in range(len(Ns)):
                    err = abs(float(Fraction(float(r["post"][t, k])) - want[t][k]))
                    worst = max(worst, err / tol)
                    assert err <= tol, (T, ls, t, k, err, tol)
            lnP = math.log(total.numerator) - math.log(total.denominator)
            assert abs(r["log_prob"] - lnP) <= tol + 4 * U * abs(lnP), (T, ls)
    print(f"worst error / tolerance: {worst:.4f}")


# ---- extended precision: an independent forward-backward ----------------------------------------------------------------
LD = np.longdouble


def _longdouble(models, seq, ls):
    """post and ln P(O | loop) from one composite transition matrix in np.longdouble: plain matrix products, scaled by
    the sums, no slot order"""
    Ns = [len(m[0]) for m in models]
    n = sum(Ns)
    at = np.concatenate([[0], np.cumsum(Ns)])
    pi = np.concatenate([np.asarray(m[0], dtype=LD) for m in models])
    B = np.concatenate([np.asarray(m[2], dtype=LD) for m in models])
    W = np.zeros((n, n), dtype=LD)
    for k, m in enumerate(models):
        W[at[k]:at[k + 1], at[k]:at[k + 1]] = np.asarray(m[1], dtype=LD)
    W = W + LD(math.exp(ls)) * pi[None, :]
    T = len(seq)
    alpha, scale = np.zeros((T, n), dtype=LD), np.zeros(T, dtype=LD)
    for t in range(T):
        x = (pi if t == 0 else alpha[t - 1] @ W) * B[:, seq[t]]
        scale[t] = x.sum()
        alpha[t] = x / scale[t]
    beta = np.ones(n, dtype=LD)
    post = np.zeros((T, len(Ns)), dtype=LD)
    for t in range(T - 1, -1, -1):
        g = alpha[t] * beta
        g = g / g.sum()
        post[t] = [g[at[k]:at[k + 1]].sum() for k in range(len(Ns))]
        if t > 0:
            beta = W @ (B[:, seq[t]] * beta)
            beta = beta / beta.sum()
    return post, np.log(scale).sum()


# (name) -> (Ns, M, T, ln_switch): positive models; computed once and shared by the two tests below
LONG_CASES = {
    "5x20_T1500": ([5] * 20, 16, 1500, -5.0),
    "21_22_7_T200": ([21, 22, 7], 8, 200, -3.0),
    "64_36_T300_never": ([64, 36], 4, 300, NINF),
    "3x5_T400_free": ([3] * 5, 6, 400, 0.0),
}
_long_cache = {}


def _long(name):
    if name not in _long_cache:
        Ns, M, T, ls = LONG_CASES[name]
        models = _models("random", Ns, M, 17)
        seq = np.random.default_rng(T).integers(0, M, T)
        _long_cache[name] = (models, seq, ls, R.posteriors_one(models, seq, ls))
    return _long_cache[name]


@pytest.mark.parametrize("name", list(LONG_CASES))
def test_extended_precision_forward_backward(name):
    models, seq, ls, r = _long(name)
    Ns, T = LONG_CASES[name][0], len(seq)
    want, lnP = _longdouble(models, seq, ls)
    assert r["status"] == 0
    err = float(np.max(np.abs(r["post"].astype(LD) - want)))
    tol = tolerance(T, max(Ns))
    print(f"{name}: worst error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    assert abs(r["log_prob"] - float(lnP)) <= tol + 4 * U * abs(float(lnP))


@pytest.mark.parametrize("name", list(LONG_CASES))
def test_rows_sum_to_one(name):
    _models_, seq, _ls, r = _long(name)
    Ns, T = LONG_CASES[name][0], len(seq)
    err = float(np.max(np.abs(r["post"].sum(axis=1) - 1.0)))
    print(f"{name}: rows sum to 1 within {err:.3e}")
    assert err <= tolerance(T, max(Ns))
    assert r["post"].min() >= 0.0


def test_without_switching_the_posterior_is_the_softmax_of_the_class_likelihoods():
    """sw = 0: no mass ever changes its class, so P(class k | O) is the same at every frame -- one row repeated"""
    models, seq, _ls, r = _long("64_36_T300_never")
    assert np.max(np.abs(r["post"] - r["post"][0])) <= tolerance(len(seq), 64)


# ---- e2vq_hmm_segment_posteriors: refusals before the device -----------------------------------------------------------
def _posteriors_c(models, ln_switch, Ns=None, K=None):
    Ns = [len(m[0]) for m in models] if Ns is None else Ns
    K = len(models) if K is None else K
    n = max(len(models), 1)
    ns = (C.c_int * n)(*Ns)
    keep = [[np.ascontiguousarray(m[i], dtype=np.float64) for m in models] for i in range(3)]
    ptr = lambda i: (C.c_void_p * n)(*[a.ctypes.data for a in keep[i]])
    sym, offs = np.zeros(8, np.uint16), np.array([0, 8], np.int64)
    return e.lib.e2vq_hmm_segment_posteriors(0, K, ns, 8, ptr(0), ptr(1), ptr(2), sym.ctypes.data, offs.ctypes.data, 1, ln_switch,
                                             None, None, None, 0)


def _bad(where, value):
    pi, A, B = (x.copy() for x in _uniform(3, 8))
    {"pi": pi, "A": A, "B": B}[where].flat[1] = value
    return pi, A, B


@pytest.mark.parametrize("case,needle", [
    ("K0", "e2vq_hmm_segment_posteriors: 0 models (at least 1)"),
    ("N0", "e2vq_hmm_segment_posteriors: model 1 has N=0 states (1 .. 64)"),
    ("N65", "e2vq_hmm_segment_posteriors: model 0 has N=65 states (1 .. 64)"),
    ("sumN", "e2vq_hmm_segment_posteriors: 4160 states in all models (at most 4096)"),
    ("negative", "HMM parameter A[1] = -0.25: not a finite non-negative number"),
    ("nan", "HMM parameter pi[1] = nan: not a finite non-negative number"),
    ("inf", "HMM parameter B[1] = inf: not a finite non-negative number"),
    ("switch_nan", "e2vq_hmm_segment_posteriors: ln_switch = nan"),
    ("switch_pos", "e2vq_hmm_segment_posteriors: ln_switch = 0.5"),
    ("slots17", "e2vq_hmm_segment_posteriors: the classes take 17 wave-slots of 64 lanes (at most 16"),
    ("slots17_packed", "e2vq_hmm_segment_posteriors: the classes take 17 wave-slots of 64 lanes (at most 16"),
])
def test_posteriors_refuses_before_the_device(case, needle):
    ok = _uniform(3, 8)
    if case == "K0":
        rc = _posteriors_c([ok], -1.0, K=0)
    elif case == "N0":
        rc = _posteriors_c([ok, ok], -1.0, Ns=[3, 0])
    elif case == "N65":
        rc = _posteriors_c([_uniform(65, 8)], -1.0)
    elif case == "sumN":
        rc = _posteriors_c([_uniform(64, 8)] * 65, -1.0)
    elif case == "negative":
        rc = _posteriors_c([ok, _bad("A", -0.25)], -1.0)
    elif case == "nan":
        rc = _posteriors_c([_bad("pi", float("nan"))], -1.0)
    elif case == "inf":
        rc = _posteriors_c([_bad("B", float("inf"))], -1.0)
    elif case == "switch_nan":
        rc = _posteriors_c([ok], float("nan"))
    elif case == "switch_pos":
        rc = _posteriors_c([ok], 0.5)
    elif case == "slots17":
        rc = _posteriors_c([_uniform(64, 8)] * 17, -1.0)
    else:
        rc = _posteriors_c([_uniform(33, 8)] * 17, -1.0)  # (561 states: two classes of 33 do not share a slot)
    assert rc == 1 and needle in _err(), _err()


def test_sixteen_slots_are_accepted_as_far_as_the_device():
    rc = _posteriors_c([_uniform(64, 8)] * 16, -1.0)
    if e.lib.e2vq_device_count() > 0:
        assert rc == 0, _err()
    else:
        assert rc == 1 and "no HIP device" in _err(), _err()


def test_python_mirror_raises_the_refusal():
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment_posteriors([_uniform(3, 8)], np.zeros(8, np.uint16), [0, 8], 1.0)
    assert "ln_switch = 1" in str(ei.value)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment_posteriors([_uniform(64, 8)] * 17, np.zeros(8, np.uint16), [0, 8], -1.0)
    assert "17 wave-slots" in str(ei.value)
    with pytest.raises(ValueError):
        hmm.segment_files(["a.hmm"], ["x.seq"], -1.0, frame_posteriors="frames")


def test_files_refuse_before_the_device(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    many = []
    for k in range(17):
        hmm.save_model(d / f"c{k:02d}.hmm", f"c{k:02d}", *_uniform(64, 16))
        many.append(str(d / f"c{k:02d}.hmm"))
    e.formats.write_seq(str(d / "x.seq"), "A", 16, np.arange(40) % 16)
    (d / "sub").mkdir()
    e.formats.write_seq(str(d / "sub" / "x.seq"), "A", 16, np.arange(40) % 16)

    def files(models, inputs, ls=-5.0, csv=None, frames=None):
        m, _k1 = hmm._strs(models)
        f, _k2 = hmm._strs(inputs)
        return e.lib.e2vq_hmm_segment_files_posteriors(m, len(models), None, f, len(inputs), 4, 45, 15, ls,
                                                       str(csv).encode() if csv else None, str(frames).encode() if frames else None)

    out = tmp_path / "out"
    assert files(many, [str(d / "x.seq")], csv=out, frames=out) == 1
    assert "e2vq_hmm_segment_files_posteriors: the classes take 17 wave-slots" in _err(), _err()
    assert files([], [str(d / "x.seq")], csv=out) == 1 and "e2vq_hmm_segment_files_posteriors: no models" in _err()
    assert files(many[:2], [str(d / "x.seq")], ls=2.0, csv=out) == 1 and "e2vq_hmm_segment_files_posteriors: ln_switch = 2" in _err()
    assert files(many[:2], [str(d / "x.seq"), str(d / "sub" / "x.seq")], frames=out) == 1 and "would both write" in _err(), _err()
    assert not out.exists()
    # the 17 classes are no obstacle without the flag: that call gets as far as the device
    m, _k1 = hmm._strs(many)
    f, _k2 = hmm._strs([str(d / "x.seq")])
    rc = e.lib.e2vq_hmm_segment_files(m, 17, None, f, 1, 4, 45, 15, -5.0, None)
    assert rc == 0 if e.lib.e2vq_device_count() > 0 else (rc == 1 and "no HIP device" in _err())


def _cli(cwd, *args):
    r = subprocess.run([EXE, "hmm", "segment", *args], cwd=cwd, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


def test_cli_flag_and_usage(tmp_path):
    rc, _out, err = _cli(tmp_path)
    assert rc == 2 and "[--posteriors [--frame-posteriors <dir>]]" in err
    assert "--switch-penalty <x <= 0 | -inf> [-c <csv dir|file.csv>]" in err
    rc, _out, err = _cli(tmp_path, "--models", "a.hmm", "--sequences", "x.seq", "--switch-penalty", "-5", "--frame-posteriors", "frames")
    assert rc == 2 and "hmm segment: --frame-posteriors <dir> needs --posteriors" in err
    rc, _out, err = _cli(tmp_path, "--models", "a.hmm", "--sequences", "x.seq", "--switch-penalty", "-5", "--posteriors", "--frame-posteriors")
    assert rc == 2 and "--frame-posteriors needs a value" in err
    assert not (tmp_path / "frames").exists()


# ---- the report: CSV columns, p= and the per-frame table from hand-made arrays -------------------------------------------
def _report(tmp_path, capfd, cls, entered, gbest, lp, ls, post, names=("whale", "noise", "ship"), frames=True):
    names_c, _k = hmm._strs(names)
    cls, entered, gbest = np.array(cls, np.uint16), np.array(entered, np.uint8), np.array(gbest, np.float64)
    post = np.ascontiguousarray(post, dtype=np.float64).reshape(len(cls), len(names))
    csv, fcsv = tmp_path / "rep" / "x.csv", tmp_path / "frames" / "x.csv"
    capfd.readouterr()
    rc = e.lib.e2vq_hmm_segment_report_posteriors(b"x.wav", len(cls), len(names), names_c, 45, 15, cls.ctypes.data, entered.ctypes.data,
                                                  gbest.ctypes.data, lp, ls, post.ctypes.data, str(csv).encode(),
                                                  str(fcsv).encode() if frames else None)
    assert rc == 0, _err()
    return csv.read_text().split("\n"), capfd.readouterr().out.split("\n"), fcsv.read_text().split("\n") if frames else None


def test_report_columns_p_field_and_frames_table(tmp_path, capfd):
    g = lambda x: "%.17g" % x
    cls = [0, 0, 0, 1, 1, 1, 1, 1, 2, 2]
    entered = [1, 0, 0, 1, 0, 1, 0, 0, 1, 0]
    gbest = [0.0, -1.0, -3.0, -6.0, -9.0, -13.5, -15.0, -19.0, -22.25, -26.0]
    rng = np.random.default_rng(3)
    post = rng.uniform(0.0, 1.0, (10, 3))
    post /= post.sum(axis=1, keepdims=True)
    rows, out, frames = _report(tmp_path, capfd, cls, entered, gbest, -30.0, -2.0, post)
    # the first eight columns: those of e2vq_hmm_segment_report for the same arrays, byte for byte
    names_c, _k = hmm._strs(("whale", "noise", "ship"))
    a, b, c = np.array(cls, np.uint16), np.array(entered, np.uint8), np.array(gbest)
    assert e.lib.e2vq_hmm_segment_report(b"x.wav", 10, 3, names_c, 45, 15, a.ctypes.data, b.ctypes.data, c.ctypes.data, -30.0, -2.0,
                                         str(tmp_path / "plain.csv").encode()) == 0
    plain_out = capfd.readouterr().out.split("\n")
    plain = (tmp_path / "plain.csv").read_text().split("\n")
    assert plain[0] == "segment,begin_frame,end_frame,begin_s,end_s,class,log_prob,log_prob_per_frame"
    assert rows[0] == plain[0] + ",posterior,min_posterior" and len(rows) == len(plain) == 6 and rows[5] == ""
    segs = [(0, 3, 0), (3, 5, 1), (5, 8, 1), (8, 10, 2)]
    want = R.segment_posteriors(cls, entered, post)
    for i, (b0, e0, k) in enumerate(segs):
        s = 0.0
        for t in range(b0, e0):
            s = s + post[t, k]
        assert want[i] == (s / (e0 - b0), post[b0:e0, k].min())
        assert rows[i + 1] == plain[i + 1] + f",{g(want[i][0])},{g(want[i][1])}"
    assert out[0] == "x.wav: T=10  segments=4  (switch penalty -2)" and out[:5] == plain_out[:5]
    for i in range(4):
        assert out[5 + i] == plain_out[5 + i] + " p=%.3f" % want[i][0]
    assert out[9].endswith("rep/x.csv saved") and out[10].endswith("frames/x.csv saved")
    assert frames[0] == "frame,begin_s,class,whale,noise,ship" and len(frames) == 12 and frames[11] == ""
    for t in range(10):
        assert frames[t + 1] == ",".join([str(t), g(t * 15 / 1000.0), ("whale", "noise", "ship")[cls[t]]] + [g(v) for v in post[t]])


def test_report_of_a_single_segment_and_of_an_empty_stream(tmp_path, capfd):
    rows, out, frames = _report(tmp_path, capfd, [1] * 4, [1, 0, 0, 0], [0.0, -1.0, -2.0, -2.5], -3.0, NINF,
                                [[0.25, 0.5, 0.25], [0.0, 1.0, 0.0], [0.5, 0.25, 0.25], [0.125, 0.75, 0.125]])
    assert rows[1] == "0,0,4,0,0.089999999999999997,noise,-3,-0.75,0.625,0.25" and rows[2] == "" and len(rows) == 3
    assert out[5] == "    0.000 - 0.090 noise p=0.625"
    assert frames[1] == "0,0,noise,0.25,0.5,0.25" and frames[4] == "3,0.044999999999999998,noise,0.125,0.75,0.125"
    rows, out, frames = _report(tmp_path, capfd, [], [], [], 0.0, -1.0, np.zeros((0, 3)))
    assert rows == ["segment,begin_frame,end_frame,begin_s,end_s,class,log_prob,log_prob_per_frame,posterior,min_posterior", ""]
    assert frames == ["frame,begin_s,class,whale,noise,ship", ""]
    assert out[0] == "x.wav: T=0  segments=0  (switch penalty -1)"
    # without a frames file name only the segment CSV is written
    _rows, out, _f = _report(tmp_path / "b", capfd, [0], [1], [0.0], -1.0, -1.0, [[1.0, 0.0, 0.0]], frames=False)
    assert not (tmp_path / "b" / "frames").exists() and out[5] == "    0.000 - 0.045 whale p=1.000"


def test_report_refuses_what_is_no_segmentation(tmp_path):
    names_c, _k = hmm._strs(["a"])
    g, post = np.zeros(2), np.ones(2)
    for cls, entered, needle in (([0, 1], [1, 0], "frame 1 names a model outside [0, 1)"), ([0, 0], [0, 1], "frame 0 does not start")):
        cls, entered = np.array(cls, np.uint16), np.array(entered, np.uint8)
        rc = e.lib.e2vq_hmm_segment_report_posteriors(b"x", 2, 1, names_c, 45, 15, cls.ctypes.data, entered.ctypes.data, g.ctypes.data,
                                                      -1.0, -1.0, post.ctypes.data, str(tmp_path / "no.csv").encode(), None)
        assert rc == 1 and "e2vq_hmm_segment_report_posteriors: " + needle in _err(), _err()
    cls, entered = np.zeros(2, np.uint16), np.array([1, 0], np.uint8)
    rc = e.lib.e2vq_hmm_segment_report_posteriors(b"x", 2, 1, names_c, 45, 15, cls.ctypes.data, entered.ctypes.data, g.ctypes.data, -1.0,
                                                  -1.0, None, str(tmp_path / "no.csv").encode(), None)
    assert rc == 1 and "bad arguments" in _err()
    assert not (tmp_path / "no.csv").exists()


def test_posteriors_library_exports():
    for name in ("e2vq_hmm_segment_posteriors", "e2vq_hmm_segment_posteriors_last_kernel_ms", "e2vq_hmm_segment_report_posteriors",
                 "e2vq_hmm_segment_files_posteriors"):
        assert hasattr(e.lib, name)
    assert callable(hmm.segment_posteriors) and callable(hmm.segment_posteriors_last_kernel_ms)
    import inspect
    params = inspect.signature(hmm.segment_files).parameters
    assert params["posteriors"].default is False and params["frame_posteriors"].default is None
    header = open(os.path.join(ROOT, "include", "ecoz2_classify.h")).read()
    for name in ("e2vq_hmm_segment_posteriors(", "e2vq_hmm_segment_posteriors_last_kernel_ms(", "e2vq_hmm_segment_report_posteriors(",
                 "e2vq_hmm_segment_files_posteriors("):
        assert name in header


# ---- compiler metadata (read as test_hmm_segment_cpu.py reads its kernels') ---------------------------------------------------
VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_posterior.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_posterior.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _meta(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    return lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))


@pytest.mark.parametrize("pattern", [r"k_hmm_loop_posteriorsILb0EE", r"k_hmm_loop_posteriorsILb1EE"])
def test_posterior_kernels_have_no_scratch_no_spill_and_fit_their_budget(asm, pattern):
    g = _meta(asm, pattern)
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
