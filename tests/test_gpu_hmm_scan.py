"""`hmm scan` on the GPU.  The definition of the feature is the oracle: every entry of the scan's matrix
is, bit for bit, what e2vq_hmm_score returns for that window's symbols passed as a sequence of their own -- mant, exp2,
status and ln P compared with np.array_equal on the raw bits, under both kernel bodies (ECOZ2_HMM_SCAN_PACK = 0 / 1) and
the host's own choice.  The file form is checked against the chain a user runs without it: ecoz2 lpc, vq quantize, the
windows written as .seq files, hmm classify (the class) and seq show -P (the %.17g log-probability)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import lpc_wavs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
BODIES = (None, "0", "1")  # the host's choice, one window per wave, packed


def _model(rng, N, M, zero_cols=()):
    row = lambda n: (lambda x: x / x.sum())(rng.uniform(0.05, 1.0, n))
    pi, A, B = row(N), np.stack([row(N) for _ in range(N)]), np.stack([row(M) for _ in range(N)])
    for c in zero_cols:
        B[:, c] = 0.0
    return pi, A, B


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _slices(streams, L, H):
    return [s[i:i + L] for s in streams for i in range(0, len(s) - L + 1, H)]


def _check(models, streams, L, H, monkeypatch, bodies=BODIES):
    sym, offs = hmm._pack(streams)
    slices = _slices(streams, L, H)
    ref = hmm.score(models, slices) if slices else None
    for body in bodies:
        if body is None:
            monkeypatch.delenv("ECOZ2_HMM_SCAN_PACK", raising=False)
        else:
            monkeypatch.setenv("ECOZ2_HMM_SCAN_PACK", body)
        got = hmm.scan(models, sym, offs, L, H)
        counts = [max(0, (len(s) - L) // H + 1) if len(s) >= L else 0 for s in streams]
        assert list(np.diff(got["win_offs"])) == counts
        assert got["mant"].shape == (len(slices), len(models))
        if not slices:
            continue
        for key in ("mant", "exp2", "status", "log_prob"):
            assert np.array_equal(_bits(got[key]), _bits(ref[key])), (key, body, L, H)
        order = np.argsort(ref["log_prob"], axis=1, kind="stable")  # hmm classify: ascending, stable, read from the end
        assert np.array_equal(got["best"], order[:, -1]), (body, L, H)
        assert np.array_equal(_bits(got["best_log_prob"]), _bits(np.take_along_axis(ref["log_prob"], order[:, -1:], 1)[:, 0]))
        if len(models) > 1:
            assert np.array_equal(got["second"], order[:, -2]), (body, L, H)
            assert np.array_equal(_bits(got["second_log_prob"]), _bits(np.take_along_axis(ref["log_prob"], order[:, -2:-1], 1)[:, 0]))
        else:
            assert (got["second"] == -1).all() and np.isneginf(got["second_log_prob"]).all()
    return ref


def _streams(rng, M, L):
    """several streams in one call: one shorter than L (when L > 1), one of exactly L, an empty one, two longer ones"""
    lens = ([L - 1] if L > 1 else []) + [L, 0, 2 * L + 5, max(3 * L + 1, 160) if L < 300 else 700]
    return [rng.integers(0, M, n).astype(np.uint16) for n in lens]


@pytest.mark.parametrize("M", [2, 64, 1024, 4096])
@pytest.mark.parametrize("N", [1, 3, 5, 16, 21, 22, 32, 64, 70])
def test_scan_equals_score_on_the_slices(N, M, monkeypatch):
    rng = np.random.default_rng(1000 * N + M)
    models = [_model(rng, N, M), _model(rng, N, M)]
    for L in (1, 2, 37, 300):
        streams = _streams(rng, M, L)
        for H in sorted({1, 7, L, L + 3}):
            _check(models, streams, L, H, monkeypatch)


@pytest.mark.parametrize("K", [1, 20])
def test_mixed_N_across_models(K, monkeypatch):
    rng = np.random.default_rng(K)
    Ns = [5] if K == 1 else [5, 16, 70, 3, 5, 64, 22, 1, 32, 21, 16, 5, 70, 3, 33, 8, 5, 12, 64, 2]
    models = [_model(rng, N, 64) for N in Ns]
    streams = [rng.integers(0, 64, n).astype(np.uint16) for n in (36, 37, 500, 90)]
    for H in (1, 7, 37, 40):
        _check(models, streams, 37, H, monkeypatch)


def test_zeros_in_B_give_status_1(monkeypatch):
    rng = np.random.default_rng(5)
    M = 64
    models = [_model(rng, 5, M, zero_cols=(3, 17)), _model(rng, 16, M), _model(rng, 40, M, zero_cols=(3,))]
    streams = [rng.integers(0, M, n).astype(np.uint16) for n in (400, 120)]
    ref = _check(models, streams, 20, 3, monkeypatch)
    st = ref["status"]
    assert (st[:, 0] == 1).any() and (st[:, 0] == 0).any() and (st[:, 1] == 0).all() and (st[:, 2] == 1).any()


def test_a_symbol_outside_the_alphabet_gives_status_2_where_it_is(monkeypatch):
    rng = np.random.default_rng(6)
    M, L, H = 64, 37, 7
    models = [_model(rng, 5, M), _model(rng, 22, M), _model(rng, 70, M)]
    clean = [rng.integers(0, M, n).astype(np.uint16) for n in (300, 80)]
    dirty = [clean[0].copy(), clean[1]]
    dirty[0][150] = M + 9
    ref_clean = _check(models, clean, L, H, monkeypatch)
    ref_dirty = _check(models, dirty, L, H, monkeypatch)
    starts = np.array([i for s in clean for i in range(0, len(s) - L + 1, H)])
    n0 = (300 - L) // H + 1
    hit = np.zeros(len(starts), bool)
    hit[:n0] = (starts[:n0] <= 150) & (150 < starts[:n0] + L)
    assert hit.any() and not hit.all()
    assert (ref_dirty["status"][hit] == 2).all() and (ref_dirty["status"][~hit] == 0).all()
    for key in ("mant", "exp2", "status", "log_prob"):
        assert np.array_equal(_bits(ref_dirty[key][~hit]), _bits(ref_clean[key][~hit]))


def test_top2_with_identical_models_and_without_the_matrix(monkeypatch):
    rng = np.random.default_rng(7)
    a, b = _model(rng, 5, 32), _model(rng, 8, 32)
    models = [a, b, a, b, a]  # ties in every window: the model given later ranks first
    streams = [rng.integers(0, 32, 300).astype(np.uint16)]
    _check(models, streams, 25, 5, monkeypatch)
    sym, offs = hmm._pack(streams)
    full = hmm.scan(models, sym, offs, 25, 5)
    top = hmm.scan(models, sym, offs, 25, 5, matrix=False)
    assert "mant" not in top
    assert set(np.unique(full["best"])) <= {3, 4} and ((full["best"] == 4) == (full["second"] == 2)).all()
    for key in ("best", "second", "best_log_prob", "second_log_prob", "win_offs"):
        assert np.array_equal(_bits(full[key]), _bits(top[key]))
    assert hmm.scan_last_kernel_ms() > 0


def test_a_window_longer_than_the_staging_area(monkeypatch):
    rng = np.random.default_rng(8)
    models = [_model(rng, 5, 16), _model(rng, 33, 16)]
    streams = [rng.integers(0, 16, 9000).astype(np.uint16)]
    _check(models, streams, 8500, 100, monkeypatch)


_TORCH_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
torch.cuda.init()  # (torch first: it has to find the device before the library opens it)
from ecoz2rs_amd import hmm
d = np.load(sys.argv[2])
models = list(zip(d["pi"], d["A"], d["B"]))
dev = torch.from_numpy(d["sym"].view(np.int16)).to("cuda:0")
torch.cuda.synchronize()
got = hmm.scan(models, dev, d["offs"], 30, 4)
np.savez(sys.argv[3], **got)
print("ok")
"""


def test_symbols_in_a_device_tensor(tmp_path):
    rng = np.random.default_rng(9)
    models = [_model(rng, 5, 64), _model(rng, 5, 64)]
    streams = [rng.integers(0, 64, n).astype(np.uint16) for n in (200, 90)]
    sym, offs = hmm._pack(streams)
    ref = hmm.scan(models, sym, offs, 30, 4)
    np.savez(tmp_path / "in.npz", pi=np.stack([m[0] for m in models]), A=np.stack([m[1] for m in models]),
             B=np.stack([m[2] for m in models]), sym=sym, offs=offs)
    r = subprocess.run([sys.executable, "-c", _TORCH_SCRIPT, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
    got = np.load(tmp_path / "out.npz")
    for key in ("mant", "exp2", "status", "log_prob", "best", "second", "win_offs"):
        assert np.array_equal(_bits(got[key]), _bits(ref[key]))


# ---- files -----------------------------------------------------------------------------------------------------------------
def test_scan_files_equal_the_four_command_chain(tmp_path):
    env = dict(os.environ)
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_GPUS", "ECOZ2_HMM_SCAN_PACK"):
        env.pop(k, None)
    P, M, L, H, W_ms, O_ms = 12, 16, 20, 6, 45, 15
    rng = np.random.default_rng(11)
    y = np.concatenate([lpc_wavs.ar_source(s, 6, 8000, 0.6) for s in (1, 2, 3)])
    lpc_wavs.write_wav(tmp_path / "sig" / "rec" / "x.wav", lpc_wavs.to_pcm(y, 16), 8000, 16)
    e.formats.write_cbook(str(tmp_path / "cb.cbook"), "_", np.hstack([np.zeros((M, 1)), rng.uniform(-0.8, 0.8, (M, P))]))
    names = ["whale", "ship", "rain"]
    models = {c: _model(rng, N, M) for c, N in zip(names, (3, 5, 7))}
    for c, m in models.items():
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)

    def run(*args):
        r = subprocess.run([EXE, *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout, r.stderr)
        return r.stdout

    geometry = ["-P", str(P), "-W", str(W_ms), "-O", str(O_ms), "--window", str(L), "--hop", str(H)]
    out = run("hmm", "scan", "--models", "hmms", "--codebook", "cb.cbook", *geometry, "-c", "scan_wav", "--signals", "sig/rec/x.wav")
    rows = (tmp_path / "scan_wav" / "x.csv").read_text().split("\n")
    assert rows[0] == "window,begin_frame,end_frame,begin_s,end_s,class,log_prob,second_class,second_log_prob"
    rows = [r.split(",") for r in rows[1:-1]]
    # the chain without scan
    run("lpc", "-P", str(P), "-W", str(W_ms), "-O", str(O_ms), "--signals", "sig/rec/x.wav")
    run("vq", "quantize", "--codebook", "cb.cbook", "--predictors", "data/predictors/rec/x.prd")
    cls, m, sym = e.formats.read_seq(str(tmp_path / "data" / "sequences" / f"M{M}" / "rec" / "x.seq"))
    assert m == M and len(rows) == (len(sym) - L) // H + 1 and len(rows) > 20
    assert f"sig/rec/x.wav: T={len(sym)}  windows={len(rows)}  (window {L} frames, hop {H})" in out
    files = []
    for i, r in enumerate(rows):
        assert [int(r[0]), int(r[1]), int(r[2])] == [i, i * H, i * H + L]
        assert r[3] == "%.17g" % (i * H * O_ms / 1000.0) and r[4] == "%.17g" % (((i * H + L - 1) * O_ms + W_ms) / 1000.0)
        assert r[5] in names and r[7] in names and r[5] != r[7]
        f = tmp_path / "slices" / f"{i:05d}.seq"
        f.parent.mkdir(exist_ok=True)
        e.formats.write_seq(str(f), r[5], M, sym[i * H:i * H + L])  # labelled with the class scan gave it
        files.append(f"slices/{i:05d}.seq")
    # hmm classify on the slices: every one is classified as the class it is labelled with
    run("hmm", "classify", "-c", "c12n.csv", "--models", "hmms", "--tt", "TEST", "-M", str(M), "--sequences", *files)
    c12n = [l.split(",") for l in (tmp_path / "c12n.csv").read_text().split("\n")[2:-1]]
    assert len(c12n) == len(rows) and all(l[2] == "*" and l[3] == "1" for l in c12n), [l for l in c12n if l[2] != "*"][:3]
    # seq show -P: the %.17g log-probability of the winner and of the runner-up
    lp = {}
    for c in names:
        text = run("seq", "show", "-P", "-L", "--hmm", f"hmms/{c}.hmm", *files)
        lp[c] = [l.split("=")[1].strip() for l in text.split("\n") if l.strip().startswith("log_prob =")]
        assert len(lp[c]) == len(rows)
    for i, r in enumerate(rows):
        assert r[6] == lp[r[5]][i] and r[8] == lp[r[7]][i], (i, r)
    # the .prd and .seq entry forms give the same CSV
    run("hmm", "scan", "--models", "hmms", "--codebook", "cb.cbook", *geometry, "-c", "scan_prd", "--predictors", "data/predictors/rec/x.prd")
    run("hmm", "scan", "--models", "hmms", *geometry, "-c", "scan_seq/x.csv", "--sequences", f"data/sequences/M{M}/rec/x.seq")
    want = (tmp_path / "scan_wav" / "x.csv").read_bytes()
    assert (tmp_path / "scan_prd" / "x.csv").read_bytes() == want
    assert (tmp_path / "scan_seq" / "x.csv").read_bytes() == want
    # the Python mirror of the file call
    hmm.scan_files([str(tmp_path / "hmms" / f"{c}.hmm") for c in sorted(names)], [str(tmp_path / "sig" / "rec" / "x.wav")], L, H,
                   codebook=tmp_path / "cb.cbook", P=P, W_ms=W_ms, O_ms=O_ms, csv=tmp_path / "scan_py")
    assert (tmp_path / "scan_py" / "x.csv").read_bytes() == want
