"""`hmm align --posteriors`, CPU side: the numpy restatement against an exact Fraction sum over every
admissible path of the chain (occupancy, the probability that a unit is visited, mean and variance of the frame it is entered
at); the laws of those quantities; log_prob and status on the bits of the E-step's restatement; the refusals of the entry
point and the CLI that come before any HIP call; the exports; the kernel's compiler metadata.  The GPU parity tests are in
test_gpu_hmm_align_posteriors.py."""
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_align_cases as cases
from . import hmm_align_posterior_restatement as PR
from . import hmm_align_restatement as AR
from . import hmm_embedded_restatement as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXE = os.path.join(CSRC, "ecoz2")
NINF = float("-inf")
U = 2.0 ** -53
M = cases.M


def _err():
    return e.lib.e2vq_last_error().decode()


def tolerances(T, Nmax):
    """(eps, occ_tol, w0_tol, mean_tol, var_tol).  First order, every term non-negative, so relative errors add.
    test_hmm_embedded_cpu.tolerances counts the roundings of one forward or backward step per state: at most r = 3 N + 28; a
    term g = ah bh or m u lies behind at most T forward steps, Z with its division, T backward steps and three products of its
    own: (2 T + 2) r roundings, a relative error of (2 T + 2) r U to first order, times 2 for the second order.  G and En add N
    such terms in a chain (N - 1 roundings), a sum over the frames adds T more, and d En, (d d) En cost two products more:
    eps = ((4 T + 4) r + 2 N + 2 T + 4) U bounds the relative error of every term and of every sum of non-negative terms here.
    occ: G <= 1, so occ_tol = eps.  w0 <= 1: w0_tol = eps.  The terms of w1 have the sign of d, |d| <= T: its error is at most
    eps T w0, the quotient w1 / w0 moves by at most 2 eps T (numerator and denominator), the division and the addition of ref
    round once each on a value <= T: mean_tol = 2 T (eps + U).  The variance w2 / w0 - q q: the quotient moves by at most 2 eps
    T^2, q q by 2 T mean_tol = 4 T^2 (eps + U), and the three operations round on values <= T^2; taking it back from begin_sd
    adds the square root's and the square's rounding: var_tol = 6 T^2 (eps + U) + 6 T^2 U.
    The worst errors observed over the cases below: 0.0044 of occ_tol, 0.0044 of w0_tol, 0.0006 of mean_tol, 0.0002 of
    var_tol."""
    r = 3 * Nmax + 28
    eps = ((4 * T + 4) * r + 2 * Nmax + 2 * T + 4) * U
    return eps, eps, eps, 2 * T * (eps + U), 6 * T * T * (eps + U) + 6 * T * T * U


SMALL = [
    ("plain", (3, 2, 3), [0, 1, 2], None, 6),
    ("first optional", (3, 2, 3), [0, 1, 2], [1, 0, 0], 5),
    ("last optional", (3, 2, 3), [0, 1, 2], [0, 0, 1], 5),
    ("middle optional", (2, 3, 2), [0, 1, 2], [0, 1, 0], 6),
    ("immediate repeat", (3, 2), [0, 0, 1], None, 6),
    ("T = the mandatory units", (3, 2, 3), [0, 1, 2], [1, 0, 0], 2),
]


def _small(case, zeros=0.0):
    name, Ns, units, opt, T = case
    models = cases.small_models(seed=len(name), Ns=Ns, zeros=zeros)
    rng = np.random.default_rng(T + len(units))
    return models, rng.integers(0, M, T), units, opt


# ---- against the exact sum over every admissible path ----------------------------------------------------------------------------------
def _exact(models, seq, units, optional, ls):
    """Fractions over every admissible path of (unit, state) pairs -> (P, occ[t][l], entry[l][t]): the probability that unit l
    holds frame t, and that unit l is entered at frame t (frame 0 for the unit the path starts in), both divided by P.  The sets
    are restated here so that the reference shares nothing with the restatement."""
    L, T = len(units), len(seq)
    opt = [bool(x) for x in optional] if optional is not None else [False] * L
    S0 = {0} | ({1} if opt[0] else set())
    F = {L - 1} | ({L - 2} if opt[L - 1] else set())
    skip = [l >= 2 and opt[l - 1] for l in range(L)]
    fr = lambda x: Fraction(float(x))
    sw = fr(math.exp(ls))
    occ = [[Fraction(0)] * L for _ in range(T)]
    entry = [[Fraction(0)] * T for _ in range(L)]
    total = [Fraction(0)]

    def walk(t, l, i, w, held, entered):
        if w == 0:
            return
        if t == T - 1:
            if l in F:
                total[0] += w
                for tt, ll in enumerate(held):
                    occ[tt][ll] += w
                for ll, tt in entered:
                    entry[ll][tt] += w
            return
        o = int(seq[t + 1])
        pi, A, B = models[units[l]]
        for j in range(len(pi)):
            walk(t + 1, l, j, w * fr(A[i][j]) * fr(B[j][o]), held + [l], entered)
        for l2 in [l + 1] + ([l + 2] if l + 2 < L and skip[l + 2] else []):
            if l2 >= L:
                continue
            pi2, _A2, B2 = models[units[l2]]
            for j in range(len(pi2)):
                walk(t + 1, l2, j, w * sw * fr(pi2[j]) * fr(B2[j][o]), held + [l2], entered + [(l2, t + 1)])

    o0 = int(seq[0])
    for l in sorted(S0):
        pi, _A, B = models[units[l]]
        for j in range(len(pi)):
            walk(0, l, j, fr(pi[j]) * fr(B[j][o0]), [l], [(l, 0)])
    P = total[0]
    assert P > 0
    return P, [[x / P for x in row] for row in occ], [[x / P for x in row] for row in entry]


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_occupancy_presence_and_entry_moments_against_the_exact_sum_over_every_path(case):
    """the tolerances are `tolerances`' (derived there, with the worst error observed); ref = 0 and ref = the Viterbi begin"""
    models, seq, units, opt = _small(case)
    T, L = len(seq), len(units)
    _eps, occ_tol, w0_tol, mean_tol, var_tol = tolerances(T, max(len(m[0]) for m in models))
    for ls in (0.0, -1.5):
        P, occ, entry = _exact(models, seq, units, opt, ls)
        va = AR.align(models, np.asarray(seq, np.uint16), [0, T], np.asarray(units, np.int32), [0, L], opt, ls)
        assert va["status"].tolist() == [0]
        vref = np.where(va["begin"] < 0, 0, va["begin"])
        for ref in (None, vref):
            got = PR.posteriors(models, seq, [0, T], units, [0, L], opt, ls, path_unit=va["unit"], ref=ref)
            assert got["status"].tolist() == [0]
            worst = [0.0] * 4
            for t in range(T):
                for l in range(L):
                    worst[0] = max(worst[0], abs(Fraction(got["occ"][0][t, l]) - occ[t][l]))
                assert got["post_path"][t] == got["occ"][0][t, va["unit"][t]]
            for l in range(L):
                w0 = sum(entry[l])
                worst[1] = max(worst[1], abs(Fraction(got["w0"][l]) - w0))
                assert got["present"][l] == got["w0"][l]
                if w0 == 0:
                    assert got["w0"][l] == 0.0 and math.isnan(got["begin_mean"][l]) and math.isnan(got["begin_sd"][l])
                    continue
                mean = sum(t * entry[l][t] for t in range(T)) / w0
                var = sum(t * t * entry[l][t] for t in range(T)) / w0 - mean * mean
                worst[2] = max(worst[2], abs(Fraction(got["begin_mean"][l]) - mean))
                worst[3] = max(worst[3], abs(Fraction(got["begin_sd"][l]) ** 2 - var))
            fr = [float(x) / tol for x, tol in zip(worst, (occ_tol, w0_tol, mean_tol, var_tol))]
            print(case[0], ls, "ref" if ref is not None else "0", "fractions of the bounds: occ %.2g w0 %.2g mean %.2g var %.2g" % tuple(fr))
            assert worst[0] <= occ_tol and worst[1] <= w0_tol and worst[2] <= mean_tol and worst[3] <= var_tol, fr


# ---- laws --------------------------------------------------------------------------------------------------------------------------------
def test_the_laws_of_occupancy_and_presence():
    eps = lambda T, models: tolerances(T, max(len(m[0]) for m in models))[0]
    for case in SMALL:
        models, seq, units, opt = _small(case)
        T, L = len(seq), len(units)
        tol = L * eps(T, models)  # (a sum over the units of values that are each within eps)
        got = PR.posteriors(models, seq, [0, T], units, [0, L], opt, -0.7)
        occ, w0 = got["occ"][0], got["w0"]
        assert np.abs(occ.sum(axis=1) - 1.0).max() <= tol, case[0]
        o = [bool(x) for x in opt] if opt is not None else [False] * L
        for l in range(L):
            if not o[l]:
                assert abs(w0[l] - 1.0) <= tol, (case[0], l)  # no admissible path can pass over a mandatory unit
            assert -tol <= w0[l] <= 1.0 + tol
        # the sets: a path starts in unit 0 or, over an optional unit 0, in unit 1; it ends in L - 1 or, before an optional last
        # unit, in L - 2: the masses of the two alternatives sum to one
        # unit 0 is entered at frame 0 or never (w0[0] is En_0[0] = G_0[0] plus zeros); its alternative is to start in unit 1
        assert w0[0] == occ[0, 0]
        if o[0]:
            assert abs(w0[0] + occ[0, 1] - 1.0) <= tol
        else:
            assert abs(w0[0] - 1.0) <= tol and occ[0, 1:].max(initial=0.0) == 0.0
        if o[L - 1]:
            assert abs(occ[T - 1, L - 1] + occ[T - 1, L - 2] - 1.0) <= tol
            assert abs(w0[L - 1] - occ[T - 1, L - 1]) <= tol  # (who enters the last unit holds the last frame)
        # the expected number of units on a path lies between the mandatory count and L
        assert sum(1 for x in o if not x) - tol <= w0.sum() <= L + tol
    # one unit: the occupancy is 1 at every frame, the unit is entered at frame 0
    model = cases.small_models(seed=4, Ns=(4,), zeros=0.0)
    seq = np.random.default_rng(6).integers(0, M, 40)
    got = PR.posteriors(model, seq, [0, 40], [0], [0, 1], None, -2.0, ref=np.array([7]))
    assert np.abs(got["occ"][0] - 1.0).max() <= eps(40, model)
    assert abs(got["w0"][0] - 1.0) <= eps(40, model) and got["begin_sd"][0] == 0.0 and got["begin_mean"][0] == 0.0
    assert got["w1"][0] == -7.0 * got["w0"][0] and got["w2"][0] == 49.0 * got["w0"][0]


def test_the_host_moments_are_the_restatements():
    rng = np.random.default_rng(12)
    w0 = rng.uniform(0, 1, 50)
    w0[[3, 9]] = 0.0
    d = rng.uniform(-40, 90, 50)
    w1, w2 = d * w0, (d * d + rng.uniform(0, 30, 50)) * w0
    w2[5] = (w1[5] / w0[5]) ** 2 * w0[5] * (1 - 1e-15)  # (a variance that rounds below zero)
    ref = rng.integers(0, 100, 50)
    for r in (None, ref):
        a, b = hmm.align_unit_moments(w0, w1, w2, r), PR.unit_moments(w0, w1, w2, r)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        assert np.isnan(a[1][[3, 9]]).all() and np.isnan(a[2][[3, 9]]).all() and a[2][5] >= 0.0


# ---- the E-step's bits ------------------------------------------------------------------------------------------------------------------
def test_log_prob_and_status_are_the_bits_of_the_embedded_restatement():
    batches = []
    for case in SMALL:
        models, seq, units, opt = _small(case, zeros=0.3)
        batches.append((models, [seq], [units], None if opt is None else [opt]))
    ev_streams, ev_transcripts, ev_optionals, kinds = cases.event_batch()
    batches.append((cases.event_models(), ev_streams, ev_transcripts, ev_optionals))
    ms, st, tr, op = cases.unlike_streams()
    batches.append((ms, st, tr, op))
    for models, streams, transcripts, optionals in batches:
        sym = np.concatenate([np.asarray(s, np.uint16) for s in streams])
        offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])])
        units = np.concatenate([np.asarray(u, np.int32) for u in transcripts])
        uoffs = np.concatenate([[0], np.cumsum([len(u) for u in transcripts])])
        opt = None if optionals is None else np.concatenate([np.asarray(o, np.uint8) for o in optionals])
        for ls in (0.0, -1.0):
            a = PR.posteriors(models, sym, offs, units, uoffs, opt, ls)
            b = ER.estep(models, sym, offs, units, uoffs, opt, ls)
            assert a["status"].tolist() == b["status"].tolist()
            assert a["log_prob"].tobytes() == b["log_prob"].tobytes()
            for s, stat in enumerate(a["status"]):
                if stat != 0:  # every entry of the stream is 0.0
                    assert not a["occ"][s].any() and not a["post_path"][offs[s]:offs[s + 1]].any()
                    assert not a["w0"][uoffs[s]:uoffs[s + 1]].any() and not a["w2"][uoffs[s]:uoffs[s + 1]].any()
    # the event batch: the first event in frame order decides
    a = PR.posteriors(cases.event_models(), *_packed(ev_streams, ev_transcripts, ev_optionals), -1.0)
    want = {"clean": 0, "M": 2, "dead": 1, "dead_M": 1, "M_dead": 2}
    assert a["status"].tolist() == [want[k] for k in kinds]


def _packed(streams, transcripts, optionals):
    sym = np.concatenate([np.asarray(s, np.uint16) for s in streams])
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    units = np.concatenate([np.asarray(u, np.int32) for u in transcripts])
    uoffs = np.concatenate([[0], np.cumsum([len(u) for u in transcripts])]).astype(np.int64)
    return sym, offs, units, uoffs, np.concatenate([np.asarray(o, np.uint8) for o in optionals])


# ---- refusals before the device -------------------------------------------------------------------------------------------------------
def _call(models, sym, offs, units, unit_offs, optional=None, ls=0.0, ref=None):
    K = len(models)
    ms = [tuple(np.ascontiguousarray(x, dtype=np.float64) for x in m) for m in models]
    ns = (C.c_int * max(K, 1))(*[len(m[0]) for m in ms])
    ptr = lambda i: (C.c_void_p * max(K, 1))(*[m[i].ctypes.data for m in ms])
    sym = np.ascontiguousarray(sym, dtype=np.uint16)
    offs, unit_offs = np.ascontiguousarray(offs, dtype=np.int64), np.ascontiguousarray(unit_offs, dtype=np.int64)
    units = np.ascontiguousarray(units, dtype=np.int32)
    opt = None if optional is None else np.ascontiguousarray(optional, dtype=np.uint8)
    ref = None if ref is None else np.ascontiguousarray(ref, dtype=np.int64)
    S = len(offs) - 1
    lp, st = np.zeros(max(S, 1)), np.zeros(max(S, 1), dtype=np.int32)
    return e.lib.e2vq_hmm_align_posteriors(0, K, ns, M, ptr(0), ptr(1), ptr(2), sym.ctypes.data, offs.ctypes.data, S, units.ctypes.data,
                                           unit_offs.ctypes.data, opt.ctypes.data if opt is not None else None, ls, None,
                                           ref.ctypes.data if ref is not None else None, None, None, None, None, None, lp.ctypes.data,
                                           st.ctypes.data, 0)


def test_what_the_estep_refuses_is_refused_and_so_are_a_seventeenth_slot_and_a_ref_outside_the_stream(monkeypatch):
    who = "e2vq_hmm_align_posteriors"
    models = cases.small_models()
    sym = np.zeros(10, np.uint16)
    for kw, msg in [
        (dict(units=[0, 1, 3], unit_offs=[0, 3]), f"{who}: stream 0, unit 2 names the class 3 outside [0, 3)"),
        (dict(units=[0, 1], unit_offs=[0, 0]), f"{who}: stream 0 has an empty transcript"),
        (dict(units=[0, 1, 2], unit_offs=[0, 3], optional=[0, 1, 1]), f"{who}: stream 0, units 1 and 2 are both optional"),
        (dict(units=[0], unit_offs=[0, 1], optional=[1]), f"{who}: stream 0: every unit of the transcript is optional"),
        (dict(units=[0], unit_offs=[0, 1], ls=0.5), f"{who}: ln_switch = 0.5"),
        (dict(units=[0], unit_offs=[0, 1], ls=NINF), f"{who}: ln_switch = -inf: a finite price"),
        (dict(units=[0, 1], unit_offs=[0, 2], ref=[0, 10]), f"{who}: stream 0, unit 1: ref = 10 outside [0, 10)"),
        (dict(units=[0, 1], unit_offs=[0, 2], ref=[-1, 0]), f"{who}: stream 0, unit 0: ref = -1 outside [0, 10)"),
    ]:
        assert _call(models, sym, [0, 10], **kw) == 1 and msg in _err(), (msg, _err())
    wide, units, stream = cases.packing("64x17")
    assert _call(wide, stream, [0, len(stream)], units, [0, len(units)]) == 1
    assert f"{who}: stream 0: the units take 17 wave-slots of 64 lanes (at most 16" in _err() and "resident body only" in _err()
    negative = [(m[0], m[1], -m[2]) for m in models]
    assert _call(negative, sym, [0, 10], [0], [0, 1]) == 1 and "HMM parameter" in _err()
    monkeypatch.setenv("ECOZ2_HMM_EMBED_A", "registers")
    assert _call(models, sym, [0, 10], [0], [0, 1]) == 1 and "ECOZ2_HMM_EMBED_A=registers: lds or global" in _err()
    monkeypatch.setenv("ECOZ2_HMM_EMBED_A", "lds")
    big, units, _opt, stream = cases.shape("64x6c_8u")  # A of six 64-state classes takes 195 KB
    assert _call(big, stream, [0, len(stream)], units, [0, len(units)]) == 1 and "A in LDS take" in _err()


def test_the_file_form_and_the_cli_refuse_before_the_device(tmp_path):
    names = ["a", "b", "bg", "c"]
    pm = cases.planted_models()
    for c, m in zip(names, [pm[0], pm[1], pm[3], pm[2]]):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)
    e.formats.write_seq(str(tmp_path / "x.seq"), "_", M, np.zeros(40, np.uint16))
    (tmp_path / "x.csv").write_text("segment,class\n0,a\n1,c\n")
    (tmp_path / "bad.csv").write_text("segment,class\n0,a\n1,zebra\n")
    files = [str(tmp_path / "hmms" / f"{c}.hmm") for c in names]
    seq, lab = [str(tmp_path / "x.seq")], [str(tmp_path / "x.csv")]
    for kw, msg in [
        (dict(filler="wind"), "e2vq_hmm_align_files_posteriors: the filler 'wind' is no model's class"),
        (dict(ln_switch=1.0), "ln_switch = 1"),
        (dict(label_filenames=[str(tmp_path / "bad.csv")]), "bad.csv:3: 'zebra' is no model's class"),
        (dict(W_ms=0), "e2vq_hmm_align_files_posteriors: window 0 ms"),
        (dict(input_filenames=seq * 2, label_filenames=lab * 2, frame_posteriors=tmp_path / "fr"), "would both write"),
    ]:
        args = dict(model_filenames=files, input_filenames=seq, label_filenames=lab, posteriors=True, csv=tmp_path / "o")
        args.update(kw)
        with pytest.raises(Exception) as err:
            hmm.align_files(**args)
        assert msg in str(err.value), (msg, str(err.value))
    assert not (tmp_path / "o").exists() and not (tmp_path / "fr").exists()
    with pytest.raises(ValueError):
        hmm.align_files(files, seq, lab, frame_posteriors=tmp_path / "fr")
    r = subprocess.run([EXE, "hmm", "align", "--models", "hmms", "--labels", "x.csv", "--sequences", "x.seq", "--frame-posteriors", "fr"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "hmm align: --frame-posteriors <dir> needs --posteriors" in r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert "[--posteriors [--frame-posteriors <dir>]]" in (r.stderr + r.stdout).split("ecoz2 hmm align")[1]


def test_the_refusals_shared_with_the_other_transcript_commands_keep_every_word(tmp_path):
    """Byte for byte, with the name of the entry point and of the label file in front: the seventeenth slot with its closing
    words, from arrays and from files (17 units of one 64-state class), and a label file without a unit."""
    uni = lambda N, m: (np.full(N, 1.0 / N), np.full((N, N), 1.0 / N), np.full((N, m), 1.0 / m))
    slots = "stream 0: the units take 17 wave-slots of 64 lanes (at most 16: the alignment posteriors have a resident body only)"
    assert _call([uni(64, M), uni(2, M)], np.zeros(8, np.uint16), [0, 8], [0] * 17, [0, 17]) == 1
    assert _err() == f"e2vq_hmm_align_posteriors: {slots}"
    for c, N in (("a", 64), ("b", 2)):
        hmm.save_model(tmp_path / f"{c}.hmm", c, *uni(N, 4))
    e.formats.write_seq(str(tmp_path / "x.seq"), "_", 4, np.zeros(8, np.uint16))
    (tmp_path / "wide.csv").write_text("class\n" + "a\n" * 17)
    (tmp_path / "empty.csv").write_text("class\n")
    files = [str(tmp_path / "a.hmm"), str(tmp_path / "b.hmm")]
    for lab, msg in (("wide.csv", f"{tmp_path / 'wide.csv'}: e2vq_hmm_align_files_posteriors: {slots}"),
                     ("empty.csv", f"{tmp_path / 'empty.csv'}: no labelled units")):
        with pytest.raises(e.Ecoz2Error):
            hmm.align_files(files, [str(tmp_path / "x.seq")], [str(tmp_path / lab)], posteriors=True, csv=tmp_path / "o")
        assert _err() == msg
    assert not (tmp_path / "o").exists()


def test_align_posteriors_library_exports():
    header = open(os.path.join(ROOT, "include", "ecoz2_classify.h")).read()
    for name in ("e2vq_hmm_align_posteriors", "e2vq_hmm_align_posteriors_last_kernel_ms", "e2vq_hmm_align_unit_moments",
                 "e2vq_hmm_align_report_posteriors", "e2vq_hmm_align_files_posteriors"):
        assert hasattr(e.lib, name) and name + "(" in header
    for fn in (hmm.align_posteriors, hmm.align_posteriors_last_kernel_ms, hmm.align_unit_moments):
        assert callable(fn)


# ---- compiler metadata (read as test_hmm_embedded_cpu.py reads the E-step's) ---------------------------------------------------------
VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_align_posterior.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_align_posterior.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _meta(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    return lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))


@pytest.mark.parametrize("pattern", [r"k_hmm_align_posteriorsILb0EE", r"k_hmm_align_posteriorsILb1EE"])
def test_the_kernel_has_no_scratch_no_spill_and_fits_its_budget(asm, pattern):
    g = _meta(asm, pattern)
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
    print(pattern, "vgpr", g("vgpr_count"), "sgpr", g("sgpr_count"))
