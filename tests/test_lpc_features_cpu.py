"""CPU tests of the LPC features of stored vectors (e2vq_lpc_features, `ecoz2 prd show --cepstrum/--predictors`): the
numpy restatement against a literal transcription of the reference's Rust functions, the exported symbol and its
argument checks, the CLI paths that need no device, and the ISA of the NC = 37 feature kernel."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import formats
from tests import lpc_features_restatement as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- literal transcription of src/lpc/lpca_r_rs.rs and src/lpc/lpca_cepstrum_rs.rs, one frame, plain Python floats ----
def _lpca_r(p, r, rc, a):
    pe = 0.0
    r0 = r[0]
    if 0.0 == r0:
        return 1, pe
    pe = r0
    a[0] = 1.0
    for k in range(1, p + 1):
        s = 0.0
        for i in range(1, k + 1):
            s -= a[k - i] * r[i]
        akk = s / pe
        rc[k] = akk
        a[k] = akk
        for i in range(1, (k >> 1) + 1):
            ai = a[i]
            aj = a[k - i]
            a[i] = ai + akk * aj
            a[k - i] = aj + akk * ai
        pe *= 1.0 - akk * akk
        if pe <= 0.0:
            return 2, pe
    return 0, pe


def _get_cepstrum(gain_ln, p, a, q, c):
    c[0] = gain_ln
    c[1] = -a[1]
    for i in range(2, p + 1):
        s = a[i]
        for k in range(1, i):
            s += float(i - k) * c[i - k] * a[k]
        c[i] = -s / float(i)
    for i in range(p + 1, q):
        s = 0.0
        for k in range(1, p + 1):
            s += float(i - k) * c[i - k] * a[k]
        c[i] = -s / float(i)


def _hand_frames(P):
    """a decaying autocorrelation, r[0] = 0, all zeros, pe <= 0 at a middle k, and a few ordinary rows"""
    rng = np.random.default_rng(P)
    rows = [0.9 ** np.arange(P + 1), np.zeros(P + 1), np.r_[0.0, rng.normal(size=P)]]
    bad = 0.8 ** np.arange(P + 1)
    bad[P // 2] = 3.0
    rows.append(bad)
    for _ in range(3):
        x = rng.normal(size=400)
        rows.append(np.array([np.dot(x[: len(x) - i], x[i:]) for i in range(P + 1)]))
    return np.array(rows)


@pytest.mark.parametrize("P,Q", [(3, 4), (7, 20), (12, 13), (12, 41)])
def test_restatement_equals_rust_transcription(P, Q):
    r = _hand_frames(P)
    f = F.features(r, Q)
    seen = set()
    for t, row in enumerate(r):
        rc, a, c = [0.0] * (P + 1), [0.0] * (P + 1), [0.0] * Q
        st, pe = _lpca_r(P, [float(v) for v in row], rc, a)
        seen.add(st)
        _get_cepstrum(F.c0(pe), P, a, Q, c)
        assert f["status"][t] == st and _bits(f["pe"][t]) == _bits(pe)
        assert np.array_equal(_bits(f["rc"][t]), _bits(rc)) and np.array_equal(_bits(f["a"][t]), _bits(a))
        assert np.array_equal(_bits(f["c"][t, 1:]), _bits(c[1:]))
        assert (math.isnan(f["c"][t, 0]) and math.isnan(c[0])) or _bits(f["c"][t, 0]) == _bits(c[0])
    assert seen == {0, 1, 2}


def test_rust_value_format():
    cases = [(0.0, "0.0000e0"), (-0.0, "-0.0000e0"), (1.2345e-6, "1.2345e-6"), (-9.99991e-6, "-9.9999e-6"),
             (1e-5, "0.00001"), (1.0, "1.00000"), (-2.5, "-2.50000"), (math.nan, "NaN"), (math.inf, "inf"),
             (-math.inf, "-inf"), (3e-300, "3.0000e-300")]
    for v, s in cases:
        assert F.rust_value(v) == s, v


def test_features_symbol_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "ecoz2_vq.h")).read()
    assert re.search(r"int e2vq_lpc_features\(int device, int P, int Q, const double \*frames, int64_t T, int32_t \*status, "
                     r"double \*pe, double \*rc,\s+double \*a, double \*c, int on_device\);", hdr)
    syms = subprocess.run(["nm", "-D", "--defined-only", e.lib_path], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T e2vq_lpc_features$", syms, re.M)


def test_features_bad_arguments_fail_before_any_device_call():
    fr = np.ones((4, 13))
    lib = e.lib
    cases = [
        ((0, 0, 0, fr.ctypes.data, 4), "out of range"),
        ((0, 81, 0, fr.ctypes.data, 4), "out of range"),
        ((0, 12, 12, fr.ctypes.data, 4), "must be > prediction order"),
        ((0, 12, 5, fr.ctypes.data, 4), "must be > prediction order"),
        ((0, 12, -1, fr.ctypes.data, 4), "must be > prediction order"),
        ((0, 12, e.lpc.MAX_Q + 1, fr.ctypes.data, 4), "exceeds the limit"),
        ((0, 12, 20, None, 4), "bad arguments"),
        ((0, 12, 20, fr.ctypes.data, -1), "bad arguments"),
    ]
    for args, msg in cases:
        assert lib.e2vq_lpc_features(*args, None, None, None, None, None, 0) != 0
        assert msg in e.lib.e2vq_last_error().decode(), (args, e.lib.e2vq_last_error().decode())
    with pytest.raises(e.Ecoz2Error, match="must be > prediction order"):
        e.lpc.features(fr, q=12)
    with pytest.raises(ValueError):
        e.lpc.features(fr, q=0, want=("c",))
    with pytest.raises(ValueError):
        e.lpc.features(fr, q=20, want=("k",))


def _show(*args, cwd=None):
    return subprocess.run([EXE, "prd", "show", *args], capture_output=True, text=True, cwd=cwd, timeout=120)


def test_cli_cepstrum_not_above_order(tmp_path):
    path = str(tmp_path / "p12.prd")
    formats.write_prd(path, "A", _hand_frames(12))
    for q in (10, 12, 0):
        r = _show("--cepstrum", str(q), path)
        out, err, _ = F.show(path, "A", 12, _hand_frames(12), cepstrum_q=q)
        assert r.returncode == 0 and r.stdout == out == f"# {path}\n"
        assert r.stderr == err == f"cepstrum value={q} must be > prediction order=12"


def test_cli_unknown_flags_print_usage(tmp_path):
    path = str(tmp_path / "p12.prd")
    formats.write_prd(path, "A", _hand_frames(12))
    for args in (["--bogus", path], ["--cepstrum", "x", path], ["--cepstrum", "-3", path], ["-f", "-1", path], []):
        r = _show(*args)
        assert r.returncode == 2 and "usage" in r.stderr and "--cepstrum" in r.stderr, args


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_isa_feature_kernel_nc37_no_scratch_and_correctly_rounded_sqrt(tmp_path):
    out = tmp_path / "feat.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-DE2VQ_LPC_NC_LIST(X)=X(37)", "-o", str(out),
                    os.path.join(ROOT, "ecoz2rs_amd", "csrc", "lpc_features.hip")], check=True, timeout=900,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = out.read_text()
    metas = [(m.group(1), m.group(2)) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S)
             if "k_feat_lane" in m.group(1)]
    assert metas and all("ILi37E" in n for n, _ in metas), [n for n, _ in metas]
    for name, meta in metas:
        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", meta).group(1))  # noqa: E731
        assert g("private_segment_fixed_size") == 0, name
        assert g("vgpr_spill_count") == 0, name
    # the double sqrt of c[0] = ln(sqrt(pe)): LLVM's correctly rounded expansion (scale into range, v_rsq_f64, Newton
    # steps with FMA residuals, rescale, class fix-up of 0 / inf), never the bare v_sqrt_f64 (not correctly rounded)
    for name, _ in metas:
        body = text[re.search(r"^" + re.escape(name) + r":", text, re.M).start():]
        body = body[:body.index("s_endpgm")]
        assert "v_sqrt_f64" not in body, name
        i = body.index("v_rsq_f64")
        seq = body[i:i + 2000]
        assert len(re.findall(r"v_fma(c)?_f64", seq)) >= 6, name
        assert "v_ldexp_f64" in seq and "v_cmp_class_f64" in seq and "0x260" in seq, name
