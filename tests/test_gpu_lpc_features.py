"""GPU tests of the LPC features of stored vectors: e2vq_lpc_features / ecoz2rs_amd.lpc.features on numpy and on torch
device tensors, and `ecoz2 prd show --cepstrum / --predictors / -k --zrs / --zrs / --pickle` on .prd and CBOR predictor
files, all against the numpy restatement (tests/lpc_features_restatement.py)."""
import math
import os
import pickle
import struct
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import formats
from tests import lpc_features_restatement as F
from tests import lpc_wavs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _hand_rows(P):
    """r[0] = 0 (status 1), all zeros (status 1), pe <= 0 at a middle k (status 2), and a decaying row"""
    rng = np.random.default_rng(100 + P)
    bad = 0.8 ** np.arange(P + 1)
    bad[max(P // 2, 1)] = 3.0
    return np.array([np.r_[0.0, rng.normal(size=P)], np.zeros(P + 1), bad, 0.9 ** np.arange(P + 1)])


def _corpus(P):
    s = lpc_wavs.to_pcm(lpc_wavs.ar_source(3, 12, 16000, 0.5), 16)
    fr, st = e.lpc.analyze(s, 16000, P=P)
    syn = e.synth.synth_frames(7, 4, P, 0, 300)
    return np.concatenate([syn, fr[st == 0][:200], _hand_rows(P)])


def _check(got, ref, c0_exact=True):
    for k in ("status", "pe", "rc", "a"):
        if k in got:
            assert np.array_equal(np.asarray(got[k]).view(np.uint64 if k != "status" else np.int32),
                                  np.asarray(ref[k]).view(np.uint64 if k != "status" else np.int32)), k
    if "c" in got:
        c, cr = np.asarray(got["c"]), ref["c"]
        # a NaN is a NaN: its payload is not part of the contract (x86 and the GPU make different ones)
        nan = np.isnan(cr)
        assert np.array_equal(np.isnan(c), nan)
        assert np.array_equal(_bits(c[:, 1:][~nan[:, 1:]]), _bits(cr[:, 1:][~nan[:, 1:]]))
        nan = nan[:, 0]
        if c0_exact:
            assert np.array_equal(_bits(c[~nan, 0]), _bits(cr[~nan, 0]))
        else:  # device log: within 1 ulp
            b, br = _bits(c[~nan, 0]).astype(np.int64), _bits(cr[~nan, 0]).astype(np.int64)
            assert np.all(np.abs(b - br) <= 1)


@pytest.mark.parametrize("P", [12, 36, 40, 7, 80])
def test_features_numpy_equals_restatement(P):
    r = _corpus(P)
    qs = sorted({P + 1, 3 * P + 5, e.lpc.MAX_Q} | ({48} if 48 > P else set()))
    for q in qs:
        ref = F.features(r, q)
        assert set(ref["status"]) == {0, 1, 2}
        got = e.lpc.features(r, q=q)
        _check(got, ref)
    # outputs left out: only c (pe is still needed on the host for c[0]), only a, only status
    ref = F.features(r, P + 1)
    _check(e.lpc.features(r, q=P + 1, want=("c",)), ref)
    _check(e.lpc.features(r, want=("a",)), ref)
    _check(e.lpc.features(r, want=("status", "rc")), ref)


def test_features_host_path_in_chunks():
    P, q = 12, 13
    r = e.synth.synth_frames(11, 4, P, 0, (1 << 18) + 77)
    r[-5] = 0.0
    ref = F.features(r, q)
    _check(e.lpc.features(r, q=q, want=("status", "c")), ref)
    assert e.lpc.features(r[:0], q=q)["c"].shape == (0, q)


_TORCH_SCRIPT = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
torch.cuda.init()
import ecoz2rs_amd as e
from tests import lpc_wavs
out = sys.argv[2]
for P in (36, 40, 7):
    s = lpc_wavs.to_pcm(lpc_wavs.ar_source(5, 12, 24000, 0.5), 16)
    fr, st = e.lpc.analyze(s, 16000, P=P, out="torch")
    x = fr[st == 0]
    hand = torch.tensor(np.load(os.path.join(out, f"hand{P}.npy")), dtype=torch.float64, device=fr.device)
    x = torch.cat([x, hand]).contiguous()
    f = e.lpc.features(x, q=48)
    assert all(v.is_cuda and v.device == fr.device for v in f.values()), "outputs left the device"
    np.save(os.path.join(out, f"in{P}.npy"), x.cpu().numpy())
    for k, v in f.items():
        np.save(os.path.join(out, f"{k}{P}.npy"), v.cpu().numpy())
print("ok")
"""


def test_features_torch_device_tensors(tmp_path):
    for P in (36, 40, 7):
        np.save(tmp_path / f"hand{P}.npy", _hand_rows(P))
    r = subprocess.run([sys.executable, "-c", _TORCH_SCRIPT, ROOT, str(tmp_path)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
    for P in (36, 40, 7):
        x = np.load(tmp_path / f"in{P}.npy")
        got = {k: np.load(tmp_path / f"{k}{P}.npy") for k in F.features(x[:1], 48)}
        _check(got, F.features(x, 48), c0_exact=False)


# ---- CLI ------------------------------------------------------------------------------------------------------------
def _show(*args, cwd=None):
    return subprocess.run([EXE, "prd", "show", *args], capture_output=True, text=True, cwd=cwd, timeout=300)


def _lpc_prd(tmp_path, P):
    sig = tmp_path / "signals" / "A" / "x.wav"
    lpc_wavs.write_wav(sig, lpc_wavs.to_pcm(lpc_wavs.ar_source(9, 12, 20000, 0.5), 16), 16000, 16)
    env = {k: v for k, v in os.environ.items() if k != "ECOZ2_VQ_OUT_ROOT"}
    r = subprocess.run([EXE, "lpc", "-P", str(P), "--signals", "signals/A/x.wav"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return str(tmp_path / "data" / "predictors" / "A" / "x.prd")


def _cbor_float(v):
    h = np.float16(v)
    if not math.isnan(v) and float(h) == v:
        return b"\xf9" + struct.pack(">e", v)
    if float(np.float32(v)) == v:
        return b"\xfa" + struct.pack(">f", v)
    return b"\xfb" + struct.pack(">d", v)


def _cbor_head(major, n):
    if n < 24:
        return bytes([major << 5 | n])
    if n < 256:
        return bytes([major << 5 | 24, n])
    if n < 65536:
        return bytes([major << 5 | 25]) + struct.pack(">H", n)
    return bytes([major << 5 | 26]) + struct.pack(">I", n)


def _write_cbor_predictor(path, cls, P, rows):
    def text(s):
        b = s.encode()
        return _cbor_head(3, len(b)) + b
    out = _cbor_head(5, 3) + text("class_name") + text(cls) + text("prediction_order") + _cbor_head(0, P)
    out += text("vectors") + _cbor_head(4, len(rows))
    for row in rows:
        out += _cbor_head(4, len(row)) + b"".join(_cbor_float(float(v)) for v in row)
    with open(path, "wb") as f:
        f.write(out)


_CASES = [
    dict(args=["--cepstrum", "20"], kw=dict(cepstrum_q=20)),
    dict(args=["--cepstrum", "48", "-f", "0"], kw=dict(cepstrum_q=48, from_=0)),
    dict(args=["--cepstrum", "20", "-t", "5"], kw=dict(cepstrum_q=20, to=5)),
    dict(args=["--cepstrum", "20", "-f", "3", "-t", "25"], kw=dict(cepstrum_q=20, from_=3, to=25)),
    dict(args=["--cepstrum", "20", "-f", "20"], kw=dict(cepstrum_q=20, from_=20)),
    dict(args=["--predictors"], kw=dict(predictors=True)),
    dict(args=["--predictors", "-f", "0", "-t", "12"], kw=dict(predictors=True, from_=0, to=12)),
    dict(args=["--predictors", "-k", "-t", "99"], kw=dict(predictors=True, reflections=True, to=99)),
    dict(args=["-k", "--zrs"], kw=dict(reflections=True)),
    dict(args=["-k", "--zrs", "-f", "0", "-t", "4"], kw=dict(reflections=True, from_=0, to=4)),
    dict(args=["--zrs"], kw=dict()),
    dict(args=["--zrs", "-f", "0"], kw=dict(from_=0)),
    dict(args=["--zrs", "-f", "13"], kw=dict(from_=13)),
]


def _check_cli(path, cls, P, rows, tmp_path):
    for case in _CASES:
        r = _show(*case["args"], path)
        out, err, sel = F.show(path, cls, P, rows, **case["kw"])
        assert r.returncode == 0, (case, r.stderr)
        assert r.stdout == out, case
        want = [ln for ln in err.splitlines() if ln]
        got = [ln for ln in r.stderr.splitlines() if ln]
        assert len(got) == len(want), case
        for g, w in zip(got, want):  # the value round-trips
            gp, wp = g.rsplit("= ", 1), w.rsplit("= ", 1)
            assert gp[0] == wp[0] and _bits(float(gp[1])) == _bits(float(wp[1])), (g, w)
        pk = tmp_path / "out.pkl"
        r = _show(*case["args"], "--pickle", str(pk), path)
        assert r.returncode == 0 and r.stdout == f"# {path}\n{len(rows)} vectors(s) saved to \"{pk}\"\n", case
        with open(pk, "rb") as f:
            loaded = pickle.load(f)
        assert len(loaded) == len(sel) and all(len(a) == len(b) for a, b in zip(loaded, sel))
        for a, b in zip(loaded, sel):
            a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
            assert np.array_equal(np.isnan(a), np.isnan(b)), case
            assert np.array_equal(_bits(a[~np.isnan(a)]), _bits(b[~np.isnan(b)])), case
    r = _show("--zrs", "-f", "5", "-t", "3", path)
    assert r.returncode != 0 and "out of bounds" in r.stderr


def test_cli_on_prd_written_by_lpc(tmp_path):
    path = _lpc_prd(tmp_path, 12)
    rows = _read_prd_rows(path)
    _check_cli(path, "A", 12, rows, tmp_path)
    # plain show keeps its own output, byte for byte
    plain = _show("-k", path).stdout
    assert plain.startswith(f"# {path}:\n# className='A'")


def _read_prd_rows(path):
    import ctypes as C

    cls = C.create_string_buffer(96)
    P, T = C.c_int(), C.c_int64()
    assert e.lib.e2vq_prd_info(path.encode(), cls, C.byref(P), C.byref(T)) == 0
    out = np.zeros((T.value, P.value + 1))
    assert e.lib.e2vq_prd_read(path.encode(), out.ctypes.data, T.value) == 0
    return out


def test_cli_hand_prd_with_failed_frames(tmp_path):
    path = str(tmp_path / "h.prd")
    rows = np.concatenate([_hand_rows(12), e.synth.synth_frames(3, 2, 12, 0, 20)])
    formats.write_prd(path, "hand", rows)
    assert set(F.lpca_r(rows)[0]) == {0, 1, 2}
    _check_cli(path, "hand", 12, rows, tmp_path)


def test_cli_cbor_predictor_f64_f32_f16(tmp_path):
    P = 12
    rows = np.concatenate([_hand_rows(P), e.synth.synth_frames(5, 2, P, 0, 10)])
    rows = np.concatenate([rows, np.float32(rows[-3:]).astype(np.float64),  # f32-exact rows
                           np.array([[1.0, 0.5, 0.25, -0.125] + [0.0] * (P - 3)])])  # f16-exact
    path = str(tmp_path / "x.cbor")
    _write_cbor_predictor(path, "cborcls", P, rows)
    raw = open(path, "rb").read()
    assert b"\xf9" in raw and b"\xfa" in raw and b"\xfb" in raw
    _check_cli(path, "cborcls", P, rows, tmp_path)
