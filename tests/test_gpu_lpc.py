"""GPU tests of the LPC front-end: batched lpca on the reference's fixture, `analyze` against the numpy restatement of the
reference's Rust analysis, `ecoz2_lpc_signals` .prd bytes, and audio -> codebook -> sequences -> HMM classification."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import formats
from tests import lpc_restatement as R
from tests import lpc_wavs
from tests.test_oracle import _load_lpca_input

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")


_TORCH_SCRIPT = r"""
import glob, os, sys
import torch
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
import numpy as np
import ecoz2rs_amd as e
parts = []
for sel in sys.argv[3].split(","):
    path = glob.glob(os.path.join(sys.argv[2], "signals", "*", sel + ".wav"))[0]
    s, sr = e.lpc.wav_read(path)
    fr, st = e.lpc.analyze(s, sr, out="torch")
    assert fr.is_cuda and fr.dtype == torch.float64 and fr.shape[1] == 37
    parts.append(fr[st == 0])
frames = torch.cat(parts).contiguous()
with e.VqSession(36, device=0) as sess:
    sess.set_frames(frames)
    sess.prepare()
    sess.init_codebook()
    sess.learn(0.05, 64)
    np.save(os.path.join(sys.argv[2], "cb_torch.npy"), sess.get_codebook())
"""


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_lpca_batch_on_reference_fixture(oracle):
    x, p = _load_lpca_input()
    rng = np.random.default_rng(0)
    X = np.stack([x, x * 0.5, np.zeros_like(x), x[::-1].copy()] + [x * rng.uniform(0.1, 2.0) for _ in range(70)])
    for P in (p, 12, 40, 80):  # lane path (12, 36, 40) and the generic path (80)
        st, pe, r, rc, a = e.lpc.lpca_batch(X, P)
        _st_n, _pe_n, _r_n, rc_n, a_n = R.lpca(X, P)
        for i in range(len(X)):
            st_o, pe_o, r_o, rc_o, a_o = oracle.lpca(X[i], P)
            assert st[i] == st_o, (P, i)
            assert np.array_equal(_bits(r[i]), _bits(r_o)), (P, i)
            assert _bits([pe[i]]) == _bits([pe_o]), (P, i)
            if st_o == 0:
                assert np.array_equal(_bits(rc[i, 1:]), _bits(rc_o[1:])) and np.array_equal(_bits(a[i]), _bits(a_o))
            else:  # the oracle leaves rc and a of a failed row unwritten: the restatement says what the kernels leave
                assert np.array_equal(_bits(rc[i]), _bits(rc_n[i])) and np.array_equal(_bits(a[i]), _bits(a_n[i])), (P, i)
        assert st[2] == 1


def _signal(seed, n, bits, order=10, silent=None):
    s = lpc_wavs.to_pcm(lpc_wavs.ar_source(seed, order, n, 0.6), bits)
    if silent:
        s[silent[0]:silent[1]] = -3
    return s


@pytest.mark.parametrize("P", [12, 36, 40, 80])
@pytest.mark.parametrize("sr,W,O", [(16000, 45, 15), (22050, 45, 15), (32000, 30, 10), (32000, 45, 15)])
def test_analyze_equals_restatement(P, sr, W, O):
    s = _signal(P * 7 + sr, sr * 2 + 123, 16, silent=(sr // 2, sr))
    frames, status = e.lpc.analyze(s, sr, P=P, W=W, O=O)
    f_r, st_r = R.analyze(s, sr, P=P, W=W, O=O)
    assert frames.shape == f_r.shape and np.array_equal(status, st_r)
    assert (status == 1).any() and (status == 0).any()
    assert np.array_equal(_bits(frames), _bits(f_r))


def test_analyze_24_and_32_bit_and_short_signal():
    for bits in (24, 32):
        s = _signal(bits, 50000, bits)
        f, st = e.lpc.analyze(s, 32000)
        f_r, st_r = R.analyze(s, 32000)
        assert np.array_equal(st, st_r) and np.array_equal(_bits(f), _bits(f_r))
    with pytest.raises(e.Ecoz2Error, match="too short"):
        e.lpc.analyze(np.ones(1000, dtype=np.int16), 32000)


def _write_corpus(root, n_classes, per_class, seed=11, n=48000, rates=(16000, 22050, 32000), bits_l=(16, 24, 32)):
    """signals/<class>/<sel>.wav: one AR source per class (orders 8-16), recordings differ in their excitation."""
    out = {}
    for c in range(n_classes):
        cls = f"C{c:02d}"
        for j in range(per_class):
            sr = rates[(c + j) % len(rates)]
            bits = bits_l[(c + 2 * j) % len(bits_l)]
            rng = np.random.default_rng(seed * 1000 + c * 100 + j)
            y = lpc_wavs.ar_source(seed * 100 + c, 8 + (c % 9), n, 0.5)  # class shape
            y = y + 0.02 * rng.standard_normal(n)
            s = lpc_wavs.to_pcm(np.roll(y, int(rng.integers(0, n))), bits)
            sel = f"{c * per_class + j:05d}"
            path = os.path.join(root, "signals", cls, sel + ".wav")
            lpc_wavs.write_wav(path, s, sr, bits)
            out[path] = (cls, sel, s, sr)
    return out


def test_lpc_signals_prd_bytes(tmp_path, monkeypatch, capfd):
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("ECOZ2_VQ_OUT_ROOT", raising=False)
    corpus = _write_corpus(str(tmp_path), 3, 3, n=40000)
    # a silent stretch in one file (frames left out), a too-short file, and a class below minpc
    path0 = sorted(corpus)[0]
    cls0, sel0, s0, sr0 = corpus[path0]
    s0 = s0.copy()
    s0[5000:15000] = 0
    bits0 = e.lpc.wav_info(path0)[2]
    lpc_wavs.write_wav(path0, s0, sr0, bits0)
    corpus[path0] = (cls0, sel0, s0, sr0)
    lpc_wavs.write_wav(tmp_path / "signals" / "C01" / "short.wav", np.ones(100, dtype=np.int16), 16000, 16)
    lpc_wavs.write_wav(tmp_path / "signals" / "Z" / "lonely.wav", s0, 16000, 16)
    files = sorted(str(p) for p in (tmp_path / "signals").rglob("*.wav"))
    e.lpc.lpc_signals(36, 45, 15, 2, 0.0, [os.path.relpath(f, tmp_path) for f in files], mintrpt=1e9)
    out = capfd.readouterr().out
    assert "Number of classes: 4" in out and "signal too short" in out and "minpc" in out
    assert not os.path.exists(tmp_path / "data" / "predictors" / "Z")
    for path, (cls, sel, s, sr) in corpus.items():
        f_r, st_r = R.analyze(s, sr)
        ref = tmp_path / "ref.prd"
        formats.write_prd(str(ref), cls, f_r[st_r == 0])
        got = tmp_path / "data" / "predictors" / cls / (sel + ".prd")
        assert got.read_bytes() == ref.read_bytes(), path
        if (st_r != 0).any():
            assert f"{(st_r != 0).sum()} frames left out" in out


def test_config5_from_audio(tmp_path, monkeypatch, oracle):
    """lpc -> vq learn (M = 64) -> vq quantize -> hmm learn / classify on 20 well-separated classes; the codebooks equal
    the oracle's on the restated frames; analyze(out="torch") frames give the same codebook through VqSession."""
    monkeypatch.chdir(tmp_path)
    n_classes, n_train, n_test = 20, 4, 2
    corpus = _write_corpus(str(tmp_path), n_classes, n_train + n_test, seed=5, n=32000)
    rows = ["tt,class,selection"]
    for path, (cls, sel, _s, _sr) in sorted(corpus.items()):
        tt = "TRAIN" if int(sel) % (n_train + n_test) < n_train else "TEST"
        rows.append(f"{tt},{cls},{sel}")
    (tmp_path / "tt.csv").write_text("\n".join(rows) + "\n")
    env = dict(os.environ, NO_COLOR="1", ECOZ2_VQ_MAX_CODEBOOK_SIZE="64")
    env.pop("ECOZ2_VQ_OUT_ROOT", None)

    def run(*args):
        r = subprocess.run([EXE, *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    run("lpc", "-P", "36", "-W", "45", "-O", "15", "--signals", "signals")
    run("vq", "learn", "-P", "36", "--predictors", "tt.csv")
    # the oracle on the restated frames of the TRAIN files, in the sorted file order of the learn
    train = sorted(f"data/predictors/{r.split(',')[1]}/{r.split(',')[2]}.prd" for r in rows[1:] if r.startswith("TRAIN"))
    by_sel = {sel: (s, sr) for _p, (_c, sel, s, sr) in corpus.items()}
    restated = []
    for f in train:
        s, sr = by_sel[os.path.basename(f)[:-4]]
        fr, st = R.analyze(s, sr)
        restated.append(fr[st == 0])
    T_all = np.concatenate(restated)
    _rc, levels_o, _cbs = oracle.learn(T_all, 0.05, 64)
    for lv in levels_o:
        _cls, _P, cb = formats.read_cbook(str(tmp_path / "data" / "codebooks" / "_" / f"eps_0.05_M_{lv['M']:04d}.cbook"))
        assert np.array_equal(_bits(cb), _bits(lv["reflections"])), lv["M"]
    # the same frames straight from the device, no .prd round trip: in a fresh process that starts torch first (as the
    # other torch-on-GPU tests do)
    sels = ",".join(os.path.basename(f)[:-4] for f in train)
    r = subprocess.run([sys.executable, "-c", _TORCH_SCRIPT, ROOT, str(tmp_path), sels], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert np.array_equal(_bits(np.load(tmp_path / "cb_torch.npy")), _bits(levels_o[-1]["reflections"]))
    run("vq", "quantize", "--codebook", "data/codebooks/_/eps_0.05_M_0064.cbook", "--predictors", "data/predictors")
    for c in range(n_classes):
        run("hmm", "learn", "-N", "5", "-M", "64", "-s", "3", "-I", "20", "--class-name", f"C{c:02d}", "--sequences",
            "tt.csv")
    out = run("hmm", "classify", "--models", "data/hmms/N5__M64_t3__a0.3_I20", "--tt", "TEST", "-M", "64", "--sequences",
              "tt.csv")
    line = [x for x in out.splitlines() if "TOTAL" in x][0]
    acc = float(line.split("%")[0].split()[-1])
    print("config 5 from audio: TEST accuracy", acc, "% over", n_classes, "classes")
    assert acc >= 50.0, out[-3000:]  # chance is 5 %
