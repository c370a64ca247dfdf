"""`hmm segment` on the GPU: cls, state, entered, the raw bits of gbest and ln P*, and status against
the numpy restatement (tests/hmm_segment_restatement.py) at the smallest shape that reaches each code path of
k_hmm_segment -- one class and several to a wave, a class that opens the next wave, mixed N, the largest resident packing
(16 waves), the first looped one (17) and a looped one whose waves take two slots each; with ln_switch = -inf against the
existing single-model kernel; the status codes; the same bits under a small back-pointer budget, from both forced bodies
and from symbols already on the device; and the three file forms against the array call."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_segment_restatement as R
from . import lpc_wavs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
NINF = float("-inf")
SETS = {
    "1": [1],
    "5": [5],
    "1_1": [1, 1],
    "5x3": [5] * 3,
    "5x13": [5] * 13,          # 12 fit a wave, the 13th opens the next
    "5x20": [5] * 20,
    "21_22_64": [21, 22, 64],  # mixed N: one class per wave next to packed ones
    "64x16": [64] * 16,        # the largest resident shape
    "64x17": [64] * 17,        # the first looped shape
    "33x20": [33] * 20,        # looped, two slots to some waves
}
LENGTHS = (0, 1, 2, 63, 64, 65, 300)
SWITCHES = (NINF, -20.0, -3.0, 0.0)
KEYS = ("cls", "state", "entered", "gbest", "log_prob", "status")


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _assert_equal(got, want, note=None):
    for key in KEYS:
        a, b = _bits(got[key]), _bits(want[key])
        assert a.dtype == b.dtype and np.array_equal(a, b), (key, note, np.flatnonzero(a != b)[:5] if a.shape == b.shape else (a.shape, b.shape))


def _init_models(Ns, M, mtype, seed=5):
    e.hmm.set_random_seed(seed)
    return [hmm.init_model(N, M, mtype) for N in Ns]


def _streams(rng, M, lengths):
    return [rng.integers(0, M, n).astype(np.uint16) for n in lengths]


@pytest.mark.parametrize("mtype", [0, 1, 2, 3])  # random, uniform (every comparison a tie), cascades (-inf in pi and A)
@pytest.mark.parametrize("M", [2, 1024])
@pytest.mark.parametrize("name", list(SETS))
def test_segment_equals_the_restatement(name, M, mtype):
    Ns = SETS[name]
    models = _init_models(Ns, M, mtype)
    rng = np.random.default_rng(len(Ns) * 1000 + M + mtype)
    streams = _streams(rng, M, LENGTHS + ((5000,) if sum(Ns) <= 100 else ()))
    sym, offs = hmm._pack(streams)
    for ls in SWITCHES:
        got = hmm.segment(models, sym, offs, ls)
        want = R.segment(models, sym, offs, ls)
        _assert_equal(got, want, ls)
        for s, segs in enumerate(got["segments"]):
            a, b = offs[s], offs[s + 1]
            ref = R.segments_of(want["cls"][a:b], want["entered"][a:b], want["gbest"][a:b], want["log_prob"][s], ls)
            assert [(g["begin"], g["end"], g["cls"]) for g in segs] == [r[:3] for r in ref]
            assert np.array_equal(_bits(np.array([g["log_prob"] for g in segs])), _bits(np.array([r[3] for r in ref])))
    assert hmm.segment_last_kernel_ms() > 0.0


@pytest.mark.parametrize("name", ["5x3", "21_22_64", "33x20"])
def test_without_switching_the_existing_viterbi_kernel_agrees(name):
    Ns = SETS[name]
    models = _init_models(Ns, 32, 0, seed=9)
    models[-1] = models[0] if Ns[-1] == Ns[0] else models[-1]  # (where it can: two classes reach the maximum)
    streams = _streams(np.random.default_rng(2), 32, (1, 2, 64, 65, 300))
    sym, offs = hmm._pack(streams)
    got = hmm.segment(models, sym, offs, NINF)
    single = [hmm.viterbi(*m, streams) for m in models]
    for s in range(len(streams)):
        lps = np.array([v["log_prob"][s] for v in single])
        k = int(np.argmax(lps))  # the lowest class reaching the maximum
        a, b = offs[s], offs[s + 1]
        assert _bits(got["log_prob"][s:s + 1])[0] == _bits(lps[k:k + 1])[0]
        assert got["cls"][a:b].tolist() == [k] * (b - a) and got["state"][a:b].tolist() == single[k]["path"][s].tolist()
        assert got["entered"][a:b].tolist() == [1] + [0] * (b - a - 1)
        assert len(got["segments"][s]) == 1


def test_segment_status_codes():
    # the fixtures of test_viterbi_status_codes, across three models
    e.hmm.set_random_seed(5)
    models = []
    for N in (5, 3, 7):
        pi, A, B = hmm.init_model(N, 8, 3)
        B[:, 5] = 0.0  # symbol 5 cannot be emitted by any state of any class
        models.append((pi, A, B))
    seqs = [np.array([1, 5, 2, 3], dtype=np.uint16), np.array([1, 2, 3], dtype=np.uint16), np.array([1, 9, 2], dtype=np.uint16),
            np.array([5], dtype=np.uint16), np.array([8], dtype=np.uint16)]
    sym, offs = hmm._pack(seqs)
    for ls in (-2.0, NINF):
        got = hmm.segment(models, sym, offs, ls)
        assert got["status"].tolist() == [1, 0, 2, 1, 2]
        assert got["log_prob"][[0, 2, 3, 4]].tolist() == [NINF] * 4 and np.isfinite(got["log_prob"][1])
        assert got["cls"][offs[2]:offs[3]].tolist() == [0xFFFF] * 3 and got["state"][offs[4]:offs[5]].tolist() == [0xFFFF]
        assert got["entered"][offs[2]:offs[3]].tolist() == [0] * 3 and got["gbest"][offs[2]:offs[3]].tolist() == [0.0, NINF, NINF]
        _assert_equal(got, R.segment(models, sym, offs, ls), ls)  # status 1 still writes the path, by the same rules


@pytest.mark.parametrize("name", ["5x13", "21_22_64", "64x17"])
def test_chunks_and_forced_bodies_give_the_same_bits(name, monkeypatch):
    Ns = SETS[name]
    M = 32
    models = _init_models(Ns, M, 0, seed=77)
    rng = np.random.default_rng(4)
    streams = _streams(rng, M, rng.integers(0, 200, 24))
    sym, offs = hmm._pack(streams)
    ls = -3.0
    one = hmm.segment(models, sym, offs, ls)
    _assert_equal(one, R.segment(models, sym, offs, ls))
    for budget in ("1", str((2 * sum(Ns) + 4) * 500)):  # one stream per launch; a few streams per launch
        monkeypatch.setenv("ECOZ2_HMM_SEGMENT_CHUNK_BYTES", budget)
        _assert_equal(hmm.segment(models, sym, offs, ls), one, budget)
    monkeypatch.delenv("ECOZ2_HMM_SEGMENT_CHUNK_BYTES")
    for body in ("resident", "looped"):  # (resident where it is possible: more than 16 waves stay looped)
        monkeypatch.setenv("ECOZ2_HMM_SEGMENT_BODY", body)
        _assert_equal(hmm.segment(models, sym, offs, ls), one, body)
    monkeypatch.setenv("ECOZ2_HMM_SEGMENT_BODY", "fast")
    with pytest.raises(e.Ecoz2Error):
        hmm.segment(models, sym, offs, ls)


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
got = hmm.segment(models, dev, d["offs"], -3.0)
got.pop("segments")
np.savez(sys.argv[3], **got)
print("ok")
"""


def test_symbols_in_a_device_tensor(tmp_path):
    models = _init_models([5, 5, 5], 64, 0, seed=3)
    streams = _streams(np.random.default_rng(9), 64, (200, 0, 90))
    sym, offs = hmm._pack(streams)
    ref = hmm.segment(models, sym, offs, -3.0)
    np.savez(tmp_path / "in.npz", pi=np.stack([m[0] for m in models]), A=np.stack([m[1] for m in models]),
             B=np.stack([m[2] for m in models]), sym=sym, offs=offs)
    r = subprocess.run([sys.executable, "-c", _TORCH_SCRIPT, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
    _assert_equal(np.load(tmp_path / "out.npz"), ref)


# ---- files -----------------------------------------------------------------------------------------------------------------
def test_segment_files_equal_the_array_call(tmp_path, capfd):
    env = dict(os.environ)
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_GPUS", "ECOZ2_HMM_SEGMENT_BODY", "ECOZ2_HMM_SEGMENT_CHUNK_BYTES"):
        env.pop(k, None)
    P, M, W_ms, O_ms, ls = 12, 16, 45, 15, -4.0
    rng = np.random.default_rng(11)
    y = np.concatenate([lpc_wavs.ar_source(s, 6, 8000, 0.6) for s in (1, 2, 3)])
    lpc_wavs.write_wav(tmp_path / "sig" / "rec" / "x.wav", lpc_wavs.to_pcm(y, 16), 8000, 16)
    e.formats.write_cbook(str(tmp_path / "cb.cbook"), "_", np.hstack([np.zeros((M, 1)), rng.uniform(-0.8, 0.8, (M, P))]))
    names = ["rain", "ship", "whale"]  # (the order in which a directory of models is resolved)
    e.hmm.set_random_seed(21)
    models = [hmm.init_model(N, M, 0) for N in (3, 5, 7)]
    for c, m in zip(names, models):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)

    def run(*args):
        r = subprocess.run([EXE, *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout, r.stderr)
        return r.stdout

    common = ["-P", str(P), "-W", str(W_ms), "-O", str(O_ms), "--switch-penalty", str(ls)]
    out = run("hmm", "segment", "--models", "hmms", "--codebook", "cb.cbook", *common, "-c", "seg_wav", "--signals", "sig/rec/x.wav")
    want = (tmp_path / "seg_wav" / "x.csv").read_bytes()
    # the symbols `vq quantize` writes for the same recording
    run("lpc", "-P", str(P), "-W", str(W_ms), "-O", str(O_ms), "--signals", "sig/rec/x.wav")
    run("vq", "quantize", "--codebook", "cb.cbook", "--predictors", "data/predictors/rec/x.prd")
    _cls, m, sym = e.formats.read_seq(str(tmp_path / "data" / "sequences" / f"M{M}" / "rec" / "x.seq"))
    assert m == M and len(sym) > 100
    # the .prd and .seq entry forms give the same CSV
    run("hmm", "segment", "--models", "hmms", "--codebook", "cb.cbook", *common, "-c", "seg_prd", "--predictors", "data/predictors/rec/x.prd")
    run("hmm", "segment", "--models", "hmms", *common, "-c", "seg_seq/x.csv", "--sequences", f"data/sequences/M{M}/rec/x.seq")
    assert (tmp_path / "seg_prd" / "x.csv").read_bytes() == want
    assert (tmp_path / "seg_seq" / "x.csv").read_bytes() == want
    # ... which is the report of the array result for those symbols, and the block the CLI printed
    got = hmm.segment(models, np.asarray(sym, dtype=np.uint16), [0, len(sym)], ls)
    _assert_equal(got, R.segment(models, np.asarray(sym), [0, len(sym)], ls))
    names_c, _k = hmm._strs(names)
    capfd.readouterr()
    assert e.lib.e2vq_hmm_segment_report(b"sig/rec/x.wav", len(sym), 3, names_c, W_ms, O_ms, got["cls"].ctypes.data,
                                         got["entered"].ctypes.data, got["gbest"].ctypes.data, float(got["log_prob"][0]), ls,
                                         str(tmp_path / "seg_arr.csv").encode()) == 0
    block = capfd.readouterr().out
    assert (tmp_path / "seg_arr.csv").read_bytes() == want
    rows = want.decode().split("\n")
    assert rows[0] == "segment,begin_frame,end_frame,begin_s,end_s,class,log_prob,log_prob_per_frame" and len(rows) == len(got["segments"][0]) + 2
    assert rows[-2].split(",")[2] == str(len(sym))
    strip = lambda text: [l for l in text.split("\n") if l and not l.endswith(" saved")]
    assert strip(block) == strip(out)[-len(strip(block)):] and strip(block)[0].startswith(f"sig/rec/x.wav: T={len(sym)}  segments=")
    # the Python mirror of the file call
    hmm.segment_files([str(tmp_path / "hmms" / f"{c}.hmm") for c in names], [str(tmp_path / "sig" / "rec" / "x.wav")], ls,
                      codebook=tmp_path / "cb.cbook", P=P, W_ms=W_ms, O_ms=O_ms, csv=tmp_path / "seg_py")
    assert (tmp_path / "seg_py" / "x.csv").read_bytes() == want
