"""`hmm segment --class-transitions --grammar-posteriors` on the GPU: the raw bits of post and
ln P(O | loop), and status, against the numpy restatement (tests/hmm_trans_posterior_restatement.py) at the smallest shape that
reaches each code path of k_hmm_loop_posteriors_trans -- one class and several to a wave, a wave with idle lanes, a class
that opens the next wave, mixed N (packed slots next to a one-class slot), 16 waves with A read from global memory, and 150
classes with both price matrices read from global memory -- under every kind of price matrix; the status codes; the same
bits under small forward-table budgets and from symbols already on the device; with every price -inf the bits of
`segment_posteriors` at -inf; the refusal of 17 slots; and the file form against the array calls and against the
--class-transitions run without the flag."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_posterior_restatement as R7
from . import hmm_trans_posterior_restatement as R
from .hmm_segment_trans_cases import UNIFORM_PRICE, random_prices

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
NINF = float("-inf")
SETS = {
    "1": [1],
    "5": [5],
    "1_1": [1, 1],
    "5x3": [5] * 3,
    "5x12": [5] * 12,          # 60 lanes of one wave, 4 idle
    "5x13": [5] * 13,          # the 13th opens a second slot
    "21_22_64": [21, 22, 64],  # packed slots next to a one-class slot
    "64x16": [64] * 16,        # 16 slots, A from global memory
    "1x150": [1] * 150,        # K = 150: w and wT from global memory; 3 slots
}
LENGTHS = (0, 1, 2, 63, 64, 65, 129, 300)
MATRICES = ("random", "never", "free", "uniform", "row", "column")
KEYS = ("post", "log_prob", "status")


def _matrix(kind, K, seed=0):
    rng = np.random.default_rng(100 + seed)
    if kind == "random":
        return random_prices(rng, K)  # a 0.2 share -inf
    if kind == "never":
        return np.full((K, K), NINF)
    if kind == "free":
        return np.zeros((K, K))
    if kind == "uniform":
        return np.full((K, K), UNIFORM_PRICE)
    lt = -rng.uniform(0.0, 6.0, (K, K))
    if kind == "row":  # a class that cannot be left
        lt[K // 2, :] = NINF
    else:  # a class entered only at frame 0
        lt[:, K // 2] = NINF
    return lt


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _assert_equal(got, want, note=None):
    for key in KEYS:
        a, b = _bits(got[key]), _bits(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape, (key, note, a.shape, b.shape)
        assert np.array_equal(a, b), (key, note, np.argwhere(a != b)[:5])


def _init_models(Ns, M, mtype, seed=5):
    hmm.set_random_seed(seed)
    return [hmm.init_model(N, M, mtype) for N in Ns]


def _streams(rng, M, lengths):
    return [rng.integers(0, M, n).astype(np.uint16) for n in lengths]


@pytest.mark.parametrize("mtype", [0, 1, 2, 3])  # random, uniform, cascades (exact zeros in pi and A)
@pytest.mark.parametrize("M", [2, 1024])
@pytest.mark.parametrize("name", list(SETS))
def test_posteriors_equal_the_restatement(name, M, mtype):
    Ns = SETS[name]
    K = len(Ns)
    models = _init_models(Ns, M, mtype)
    rng = np.random.default_rng(K * 1000 + M + mtype)
    sym, offs = hmm._pack(_streams(rng, M, LENGTHS))
    for mk in MATRICES:
        lt = _matrix(mk, K, mtype)
        got = hmm.segment_trans_posteriors(models, sym, offs, lt)
        _assert_equal(got, R.posteriors(models, sym, offs, lt), mk)
        assert got["post"].shape == (offs[-1], K)
    if sum(Ns) <= 100:  # 3000 frames: unscaled arithmetic underflows there
        seq = _streams(rng, M, (3000,))[0]
        for mk in ("random", "column"):
            lt = _matrix(mk, K, 7)
            _assert_equal(hmm.segment_trans_posteriors(models, seq, [0, 3000], lt), R.posteriors(models, seq, [0, 3000], lt), mk)
    assert hmm.segment_trans_posteriors_last_kernel_ms() > 0.0


def test_status_codes():
    # the fixtures of test_posteriors_status_codes, under a random matrix
    hmm.set_random_seed(5)
    models = []
    for N in (5, 3, 7):
        pi, A, B = hmm.init_model(N, 8, 3)
        B[:, 5] = 0.0  # symbol 5 cannot be emitted by any state of any class
        models.append((pi, A, B))
    seqs = [np.array([1, 5, 2, 3], dtype=np.uint16), np.array([1, 2, 3], dtype=np.uint16), np.array([1, 9, 2], dtype=np.uint16),
            np.array([5], dtype=np.uint16), np.array([8], dtype=np.uint16), np.array([5, 1, 2], dtype=np.uint16),
            np.array([9, 5, 1], dtype=np.uint16), np.array([5, 9], dtype=np.uint16)]
    sym, offs = hmm._pack(seqs)
    for lt in (random_prices(np.random.default_rng(1), 3), np.full((3, 3), NINF)):
        got = hmm.segment_trans_posteriors(models, sym, offs, lt)
        # (the first event in frame order decides: [9, 5, ..] is 2, [5, 9] is 1)
        assert got["status"].tolist() == [1, 0, 2, 1, 2, 1, 2, 1]
        assert got["log_prob"][[0, 2, 3, 4, 5, 6, 7]].tolist() == [NINF] * 7 and np.isfinite(got["log_prob"][1])
        for s in (0, 2, 3, 4, 5, 6, 7):
            rows = got["post"][offs[s]:offs[s + 1]]
            assert rows.shape == (len(seqs[s]), 3) and not rows.any() and not np.signbit(rows).any()
        ok = got["post"][offs[1]:offs[2]]
        assert np.max(np.abs(ok.sum(axis=1) - 1.0)) <= 4 * 7 * (2 * 7 + 2 * 3 + 32) * 2.0 ** -53
        _assert_equal(got, R.posteriors(models, sym, offs, lt))


@pytest.mark.parametrize("name", ["5x13", "21_22_64", "64x16"])
def test_chunk_budgets_give_the_same_bits(name, monkeypatch):
    Ns = SETS[name]
    M = 32
    models = _init_models(Ns, M, 0, seed=77)
    rng = np.random.default_rng(4)
    streams = _streams(rng, M, list(range(0, 198, 9)) + [199, 100])  # 24 streams of 0 .. 199 frames
    sym, offs = hmm._pack(streams)
    lt = _matrix("random", len(Ns), 2)
    one = hmm.segment_trans_posteriors(models, sym, offs, lt)
    _assert_equal(one, R.posteriors(models, sym, offs, lt))
    slots = R.packing(Ns)[2]
    for budget in ("1", str(8 * (sum(Ns) + slots) * 500)):  # one stream per launch; a few streams per launch (a0 != 0)
        monkeypatch.setenv("ECOZ2_HMM_POSTERIOR_CHUNK_BYTES", budget)
        _assert_equal(hmm.segment_trans_posteriors(models, sym, offs, lt), one, budget)


@pytest.mark.parametrize("name", ["5x3", "5x13", "21_22_64", "64x16"])
def test_all_prices_minus_infinity_are_the_bits_of_the_single_price_kernel(name):
    Ns = SETS[name]
    models = _init_models(Ns, 32, 0, seed=9)
    sym, offs = hmm._pack(_streams(np.random.default_rng(2), 32, (0, 1, 2, 64, 65, 300)))
    got = hmm.segment_trans_posteriors(models, sym, offs, np.full((len(Ns),) * 2, NINF))
    _assert_equal(got, hmm.segment_posteriors(models, sym, offs, NINF))
    _assert_equal(got, R7.posteriors(models, sym, offs, NINF))


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
got = hmm.segment_trans_posteriors(models, dev, d["offs"], d["lt"])
np.savez(sys.argv[3], **got)
print("ok")
"""


def test_symbols_in_a_device_tensor(tmp_path):
    models = _init_models([5, 5, 5], 64, 0, seed=3)
    streams = _streams(np.random.default_rng(9), 64, (200, 0, 90))
    sym, offs = hmm._pack(streams)
    lt = _matrix("random", 3, 5)
    ref = hmm.segment_trans_posteriors(models, sym, offs, lt)
    _assert_equal(ref, R.posteriors(models, sym, offs, lt))
    np.savez(tmp_path / "in.npz", pi=np.stack([m[0] for m in models]), A=np.stack([m[1] for m in models]),
             B=np.stack([m[2] for m in models]), sym=sym, offs=offs, lt=lt)
    r = subprocess.run([sys.executable, "-c", _TORCH_SCRIPT, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
    _assert_equal(np.load(tmp_path / "out.npz"), ref)


def test_seventeen_slots_are_refused():
    models = _init_models([64] * 17, 4, 1)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment_trans_posteriors(models, np.zeros(8, np.uint16), [0, 8], np.zeros((17, 17)))
    assert "17 wave-slots" in str(ei.value)


# ---- files -----------------------------------------------------------------------------------------------------------------
def test_segment_files_with_grammar_posteriors_equal_the_array_calls(tmp_path):
    env = dict(os.environ)
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_GPUS", "ECOZ2_HMM_SEGMENT_BODY", "ECOZ2_HMM_SEGMENT_CHUNK_BYTES",
              "ECOZ2_HMM_POSTERIOR_CHUNK_BYTES", "ECOZ2_HMM_POSTERIOR_BODY"):
        env.pop(k, None)
    M, W_ms, O_ms, ls = 16, 45, 15, -1.5
    names = ["rain", "ship", "whale"]  # (the order in which a directory of models is resolved)
    hmm.set_random_seed(21)
    models = []
    for k, N in enumerate((3, 5, 7)):  # class k prefers the symbols 5 k .. 5 k + 4, so that the stream below has segments
        pi, A, B = hmm.init_model(N, M, 0)
        B[:, 5 * k:5 * k + 5] *= 20.0
        models.append((pi, A, B / B.sum(axis=1, keepdims=True)))
    for c, m in zip(names, models):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)
    file_lt = np.array([[-0.5, -3.0, NINF], [-2.0, -0.25, -1.0], [NINF, -4.0, -0.125]])
    hmm.write_class_transitions(tmp_path / "t.csv", names, file_lt)
    rng = np.random.default_rng(12)
    sym = np.concatenate([5 * k + rng.integers(0, 5, n) for k, n in ((0, 130), (1, 90), (2, 100), (1, 80))]).astype(np.uint16)
    T = len(sym)
    e.formats.write_seq(str(tmp_path / "x.seq"), "rain", M, sym)

    def run(*args):
        r = subprocess.run([EXE, *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout, r.stderr)
        return r.stdout

    common = ["hmm", "segment", "--models", "hmms", "-W", str(W_ms), "-O", str(O_ms), "--switch-penalty", str(ls), "--sequences", "x.seq",
              "--class-transitions", "t.csv"]
    plain_out = run(*common, "-c", "plain")
    assert not (tmp_path / "frames").exists()
    out = run(*common, "-c", "post", "--grammar-posteriors", "--frame-posteriors", "frames")
    plain = (tmp_path / "plain" / "x.csv").read_bytes()
    want = (tmp_path / "post" / "x.csv").read_text().split("\n")
    frames = (tmp_path / "frames" / "x.csv").read_text().split("\n")
    # the first eight columns are the --class-transitions run's, byte for byte
    rows = plain.decode().split("\n")
    assert len(want) == len(rows) and want[0] == rows[0] + ",posterior,min_posterior"
    assert [",".join(r.split(",")[:8]) for r in want[1:-1]] == rows[1:-1] and want[-1] == ""
    # the new columns and the per-frame table: those computed from the array calls under the effective prices
    lt = file_lt + ls
    seg = hmm.segment_trans(models, sym, [0, T], lt)
    post = hmm.segment_trans_posteriors(models, sym, [0, T], lt)
    _assert_equal(post, R.posteriors(models, sym, [0, T], lt))
    g = lambda v: "%.17g" % v
    stats = R7.segment_posteriors(seg["cls"], seg["entered"], post["post"])
    assert len(stats) == len(want) - 2 and len(stats) > 1
    assert [r.split(",")[8:] for r in want[1:-1]] == [[g(a), g(b)] for a, b in stats]
    assert frames[0] == "frame,begin_s,class,rain,ship,whale" and len(frames) == T + 2 and frames[-1] == ""
    for t in range(T):
        assert frames[t + 1] == ",".join([str(t), g(t * O_ms / 1000.0), names[seg["cls"][t]]] + [g(v) for v in post["post"][t]])
    # the block: the flag-less lines with p= on each segment line
    strip = lambda text: [l for l in text.split("\n") if l and not l.endswith(" saved")]
    a, b = strip(plain_out), strip(out)
    n = len(stats)
    assert len(a) == len(b) and a[:-n] == b[:-n]
    assert b[-n:] == [x + " p=%.3f" % s[0] for x, s in zip(a[-n:], stats)]
    # without --frame-posteriors only the CSV is written; the Python mirror of the file call
    run(*common, "-c", "post2", "--grammar-posteriors")
    assert (tmp_path / "post2" / "x.csv").read_text().split("\n") == want
    files = [str(tmp_path / "hmms" / f"{c}.hmm") for c in names]
    hmm.segment_files(files, [str(tmp_path / "x.seq")], ls, W_ms=W_ms, O_ms=O_ms, csv=tmp_path / "py", class_transitions=tmp_path / "t.csv",
                      grammar_posteriors=True, frame_posteriors=tmp_path / "py_frames")
    assert (tmp_path / "py" / "x.csv").read_text().split("\n") == want
    assert (tmp_path / "py_frames" / "x.csv").read_text().split("\n") == frames
    hmm.segment_files(files, [str(tmp_path / "x.seq")], ls, W_ms=W_ms, O_ms=O_ms, csv=tmp_path / "py_plain",
                      class_transitions=tmp_path / "t.csv")
    assert (tmp_path / "py_plain" / "x.csv").read_bytes() == plain
