"""`hmm transitions --em` on the GPU: every limb of the count table, the raw bits of ln P(O | loop) and the
status against the numpy restatement (tests/hmm_transitions_em_restatement.py) at the smallest shape that reaches each code path
of k_hmm_trans_estep -- one class and several to a wave, a wave with idle lanes, a class that opens the next wave, mixed N, 16
waves with A read from global memory, and 150 classes with both price matrices and the count table in global memory -- under
every kind of price matrix; ln P and status against `segment_trans_posteriors` on the GPU; the status fixtures; a call of
several streams against the calls per stream; both routes of the count table; a small forward-table budget; symbols already
on the device; three iterations of the training; the file form against the array calls, and its file read by `hmm segment`;
the refusal of 17 slots."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_transitions_em_restatement as R
from .hmm_segment_trans_cases import random_prices

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
    "1x150": [1] * 150,        # K = 150: w, wT and the C table in global memory; 3 slots
}
LENGTHS = (0, 1, 2, 63, 64, 65, 129, 300)
MATRICES = ("random", "never", "free", "row", "column")
ENV = ("ECOZ2_HMM_TRANS_EM_C", "ECOZ2_HMM_POSTERIOR_CHUNK_BYTES")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _matrix(kind, K, seed=0):
    rng = np.random.default_rng(100 + seed)
    if kind == "random":
        return random_prices(rng, K)  # a 0.2 share -inf
    if kind == "never":
        return np.full((K, K), NINF)
    if kind == "free":
        return np.zeros((K, K))
    lt = -rng.uniform(0.0, 6.0, (K, K))
    if kind == "row":  # a class that cannot be left
        lt[K // 2, :] = NINF
    else:  # a class entered only at frame 0
        lt[:, K // 2] = NINF
    return lt


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _assert_equal(got, want, note=None, keys=("acc", "log_prob", "status")):
    for key in keys:
        a, b = _bits(got[key]), _bits(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape, (key, note, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (key, note, np.argwhere(a != b)[:5])


def _init_models(Ns, M, mtype, seed=5):
    hmm.set_random_seed(seed)
    return [hmm.init_model(N, M, mtype) for N in Ns]


def _streams(rng, M, lengths):
    return [rng.integers(0, M, n).astype(np.uint16) for n in lengths]


@pytest.mark.parametrize("M,mtype", [(2, 3), (1024, 0)])  # cascades (exact zeros in pi and A) at M = 2, random models at 1024
@pytest.mark.parametrize("name", list(SETS))
def test_counts_equal_the_restatement(name, M, mtype):
    Ns = SETS[name]
    K = len(Ns)
    models = _init_models(Ns, M, mtype)
    rng = np.random.default_rng(K * 1000 + M + mtype)
    sym, offs = hmm._pack(_streams(rng, M, LENGTHS))
    for mk in MATRICES:
        lt = _matrix(mk, K, mtype)
        got = hmm.transitions_estep(models, sym, offs, lt)
        _assert_equal(got, R.estep(models, sym, offs, lt), mk)
        assert got["acc"].shape == (2 * K * K + 2,) and got["acc"][-2:].tolist() == [len(LENGTHS), 0]
        if mk == "never":
            assert not got["acc"][:-2].any()
        _assert_equal(got, hmm.segment_trans_posteriors(models, sym, offs, lt), mk, keys=("log_prob", "status"))
    assert hmm.transitions_estep_last_kernel_ms() > 0.0


def test_status_fixtures_add_nothing_and_are_counted_as_skipped():
    hmm.set_random_seed(5)
    models = []
    for N in (5, 3, 7):
        pi, A, B = hmm.init_model(N, 8, 3)
        B[:, 5] = 0.0  # symbol 5 cannot be emitted by any state of any class
        models.append((pi, A, B))
    rng = np.random.default_rng(3)
    clean = [np.array([1, 2, 3, 4, 6, 7, 0, 1] * n, dtype=np.uint16) for n in (20, 9)]
    bad = [np.array([1, 5, 2, 3], dtype=np.uint16), np.array([1, 9, 2], dtype=np.uint16), np.array([5], dtype=np.uint16),
           np.array([8], dtype=np.uint16), np.array([1, 2, 3, 4, 6, 7, 0, 1] * 10 + [5, 1], dtype=np.uint16),
           np.array([1, 2, 3, 4, 6, 7] * 12 + [9], dtype=np.uint16)]
    lt = random_prices(rng, 3)
    sym_c, offs_c = hmm._pack(clean)
    first = hmm.transitions_estep(models, sym_c, offs_c, lt)  # clean streams first: the reused buffers hold data
    assert first["status"].tolist() == [0, 0] and first["acc"][:-2].any() and first["acc"][-2:].tolist() == [2, 0]
    sym, offs = hmm._pack(clean + bad)
    got = hmm.transitions_estep(models, sym, offs, lt)
    assert got["status"].tolist() == [0, 0, 1, 2, 1, 2, 1, 2]
    assert (got["log_prob"][2:] == NINF).all() and np.isfinite(got["log_prob"][:2]).all()
    assert got["acc"][-2:].tolist() == [2, 6] and np.array_equal(got["acc"][:-2], first["acc"][:-2])
    _assert_equal(got, R.estep(models, sym, offs, lt))
    only_bad = hmm.transitions_estep(models, *hmm._pack(bad), lt)
    assert not only_bad["acc"][:-2].any() and only_bad["acc"][-2:].tolist() == [0, 6]


@pytest.mark.parametrize("name", ["5x13", "21_22_64", "64x16"])
def test_one_call_a_call_per_stream_both_routes_and_chunk_budgets_give_the_same_limbs(name, monkeypatch):
    Ns = SETS[name]
    K, M = len(Ns), 32
    models = _init_models(Ns, M, 0, seed=77)
    rng = np.random.default_rng(4)
    streams = _streams(rng, M, list(range(0, 198, 18)) + [199, 100])  # 13 streams of 0 .. 199 frames
    sym, offs = hmm._pack(streams)
    lt = _matrix("random", K, 2)
    one = hmm.transitions_estep(models, sym, offs, lt)
    _assert_equal(one, R.estep(models, sym, offs, lt))
    # a call per stream, summed on the host: into one array, which the calls add to and never clear
    acc = np.zeros(hmm.transitions_acc_words(K), dtype=np.int64)
    for s in streams:
        r = hmm.transitions_estep(models, s, [0, len(s)], lt, acc=acc)
        assert r["acc"] is acc
    assert np.array_equal(acc, one["acc"])
    for route in ("global", "lds"):
        monkeypatch.setenv("ECOZ2_HMM_TRANS_EM_C", route)
        _assert_equal(hmm.transitions_estep(models, sym, offs, lt), one, route)
    monkeypatch.delenv("ECOZ2_HMM_TRANS_EM_C")
    slots = R.packing(Ns)[2]
    for budget in ("1", str(8 * (sum(Ns) + slots) * 500)):  # one stream per launch; a few streams per launch (a0 != 0)
        monkeypatch.setenv("ECOZ2_HMM_POSTERIOR_CHUNK_BYTES", budget)
        _assert_equal(hmm.transitions_estep(models, sym, offs, lt), one, budget)


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
got = hmm.transitions_estep(models, dev, d["offs"], d["lt"])
np.savez(sys.argv[3], **got)
print("ok")
"""


def test_symbols_in_a_device_tensor(tmp_path):
    models = _init_models([5, 5, 5], 64, 0, seed=3)
    streams = _streams(np.random.default_rng(9), 64, (200, 0, 90))
    sym, offs = hmm._pack(streams)
    lt = _matrix("random", 3, 5)
    ref = hmm.transitions_estep(models, sym, offs, lt)
    _assert_equal(ref, R.estep(models, sym, offs, lt))
    np.savez(tmp_path / "in.npz", pi=np.stack([m[0] for m in models]), A=np.stack([m[1] for m in models]),
             B=np.stack([m[2] for m in models]), sym=sym, offs=offs, lt=lt)
    r = subprocess.run([sys.executable, "-c", _TORCH_SCRIPT, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
    _assert_equal(np.load(tmp_path / "out.npz"), ref)


def _corpus(M=16):
    """three classes that prefer symbols of their own, and three streams of segments in the order 0 1 2 0 1 2 ..."""
    hmm.set_random_seed(21)
    models = []
    for k, N in enumerate((3, 5, 7)):
        pi, A, B = hmm.init_model(N, M, 0)
        B[:, 5 * k:5 * k + 5] *= 20.0
        models.append((pi, A, B / B.sum(axis=1, keepdims=True)))
    rng = np.random.default_rng(12)
    streams = []
    for n_seg in (9, 6, 12):
        parts = [5 * (i % 3) + rng.integers(0, 5, int(rng.integers(12, 30))) for i in range(n_seg)]
        streams.append(np.concatenate(parts).astype(np.uint16))
    return models, streams


def test_three_iterations_of_the_training_equal_the_restatements_loop():
    models, streams = _corpus()
    sym, offs = hmm._pack(streams)
    start = np.log(np.array([[0.2, 0.5, 0.3], [0.3, 0.3, 0.4], [0.6, 0.1, 0.3]]))
    start[1, 0] = NINF  # a forbidden succession: it stays forbidden
    seen = []
    for ln_p, alpha in ((None, 0.0), (start, 0.5)):
        got, hist = hmm.train_transitions(models, sym, offs, ln_p, ln_switch=-1.5, alpha=alpha, val_auto=1e-6, max_iterations=3,
                                          callback=lambda v, x: seen.append((v, x)))
        want, whist = R.train(models, sym, offs, ln_p, ln_switch=-1.5, alpha=alpha, val_auto=1e-6, max_iterations=3)
        assert len(hist) == len(whist) == 3 and np.array_equal(_bits(hist), _bits(np.array(whist)))
        assert np.array_equal(_bits(got), _bits(want)), (got, want)
        assert seen[-3:] == [("sum_log_prob", v) for v in whist]
        assert hist[1] >= hist[0] and hist[2] >= hist[1] - 1e-9 * abs(hist[1])
    assert got[1, 0] == NINF
    # no stream of status 0: the call fails and names it
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.train_transitions(models, np.array([16, 3], dtype=np.uint16), [0, 2], start, ln_switch=-1.5)
    assert "no stream can be explained" in str(ei.value)


def test_seventeen_slots_are_refused():
    models = _init_models([64] * 17, 4, 1)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.transitions_estep(models, np.zeros(8, np.uint16), [0, 8], np.zeros((17, 17)))
    assert "17 wave-slots" in str(ei.value)


# ---- files -----------------------------------------------------------------------------------------------------------------
def test_the_file_form_equals_the_array_calls_and_its_file_is_read_by_segment(tmp_path):
    env = dict(os.environ)
    for k in ENV + ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_GPUS", "ECOZ2_HMM_SEGMENT_BODY", "ECOZ2_HMM_SEGMENT_CHUNK_BYTES", "ECOZ2_VQ_QUIET"):
        env.pop(k, None)
    M, ls = 16, -1.5
    names = ["rain", "ship", "whale"]  # (the order in which a directory of models is resolved)
    models, streams = _corpus(M)
    for c, m in zip(names, models):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)
    seqs = []
    for i, s in enumerate(streams):
        seqs.append(f"s{i}.seq")
        e.formats.write_seq(str(tmp_path / seqs[-1]), "rain", M, s)

    def run(*args):
        r = subprocess.run([EXE, *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout, r.stderr)
        return r.stdout, r.stderr

    out, err = run("hmm", "transitions", "--em", "-m", "hmms", "--switch-penalty", str(ls), "--alpha", "0.5", "-a", "1e-6", "-I", "3",
                   "-o", "t.csv", "--sequences", *seqs)
    assert "3 E-step(s); t.csv saved (alpha 0.5, 3 classes); t.csv.em.csv saved" in out and err == ""
    sym, offs = hmm._pack(streams)
    want, hist = hmm.train_transitions(models, sym, offs, None, ln_switch=ls, alpha=0.5, val_auto=1e-6, max_iterations=3)
    assert np.array_equal(_bits(hmm.read_class_transitions(tmp_path / "t.csv", names)), _bits(want))
    g = lambda v: "%.17g" % v
    assert (tmp_path / "t.csv.em.csv").read_text() == "iteration,sum_log_prob,streams_used,streams_skipped\n" + "".join(
        f"{i},{g(v)},3,0\n" for i, v in enumerate(hist))
    # --init: the file just written is a start as good as any; the Python mirror of the file call
    files = [str(tmp_path / "hmms" / f"{c}.hmm") for c in names]
    hmm.learn_transitions_files(files, [str(tmp_path / s) for s in seqs], tmp_path / "t2.csv", ls, init=tmp_path / "t.csv", alpha=0.5,
                                val_auto=1e-6, max_iterations=1)
    want2, _h = hmm.train_transitions(models, sym, offs, want, ln_switch=ls, alpha=0.5, val_auto=1e-6, max_iterations=1)
    assert np.array_equal(_bits(hmm.read_class_transitions(tmp_path / "t2.csv", names)), _bits(want2))
    # `hmm segment --class-transitions` reads the file as it is
    run("hmm", "segment", "--models", "hmms", "--switch-penalty", str(ls), "--sequences", seqs[0], "--class-transitions", "t.csv", "-c", "seg")
    rows = (tmp_path / "seg" / "s0.csv").read_text().split("\n")
    assert len(rows) > 4 and rows[-1] == ""
