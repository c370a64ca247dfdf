"""`hmm learn --loop` on the GPU: every limb of every class block, every limb of the grammar table, the raw
bits of ln P(O | loop) and the status against the numpy restatement (tests/hmm_loop_em_restatement.py) at the smallest shape
that reaches each code path of k_hmm_loop_estep -- one class and several to a wave, a wave with idle lanes, a class that opens
the next wave, mixed N, 16 waves with A and the AN table in global memory, and 150 classes with both price matrices and the
C table in global memory -- under every kind of price matrix; the grammar limbs against `transitions_estep` and ln P against
`segment_trans_posteriors` on the GPU; acc_trans = None; the status fixtures; a call of several streams against the calls per
stream; both routes of both tables; small forward-table budgets; symbols already on the device; three iterations of the
training with and without the matrix and with a frozen class; the file form against the array calls, and its files read by
`hmm segment`; the refusal of 17 slots."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_loop_em_restatement as R
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
    "64x16": [64] * 16,        # 16 slots, A and the AN table in global memory
    "1x150": [1] * 150,        # K = 150: w, wT and the C table in global memory; 3 slots
}
LENGTHS = (0, 1, 2, 63, 64, 65, 129, 300)
MATRICES = ("random", "never", "free", "row", "column")
ENV = ("ECOZ2_HMM_LOOP_EM_AN", "ECOZ2_HMM_LOOP_EM_C", "ECOZ2_HMM_TRANS_EM_C", "ECOZ2_HMM_POSTERIOR_CHUNK_BYTES")


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


def _assert_equal(got, want, note=None, keys=("acc", "acc_trans", "log_prob", "status")):
    for key in keys:
        if key == "acc":
            assert len(got[key]) == len(want[key])
            for k, (a, b) in enumerate(zip(got[key], want[key])):
                assert a.dtype == b.dtype == np.int64 and a.shape == b.shape, (key, k, note)
                assert np.array_equal(a, b), (key, k, note, np.argwhere(a != b)[:5])
            continue
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
        got = hmm.loop_estep(models, sym, offs, lt, acc_trans=True)
        want = R.estep(models, sym, offs, lt, acc_trans=True)
        _assert_equal(got, want, mk)
        lay = [R.layout(N, M) for N in Ns]
        assert all(a[l["used"]] == len(LENGTHS) and a[l["skipped"]] == 0 for a, l in zip(got["acc"], lay))
        if mk == "never":
            assert not got["acc_trans"][:-2].any()
        # the grammar limbs and ln P: the sibling passes on the GPU
        _assert_equal(got, dict(acc_trans=hmm.transitions_estep(models, sym, offs, lt)["acc"]), mk, keys=("acc_trans",))
        _assert_equal(got, hmm.segment_trans_posteriors(models, sym, offs, lt), mk, keys=("log_prob", "status"))
        # without the grammar table: the same state limbs
        plain = hmm.loop_estep(models, sym, offs, lt)
        assert "acc_trans" not in plain
        _assert_equal(plain, got, mk, keys=("acc", "log_prob", "status"))
    assert hmm.loop_estep_last_kernel_ms() > 0.0


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
    lay = [R.layout(N, 8) for N in (5, 3, 7)]
    first = hmm.loop_estep(models, *hmm._pack(clean), lt, acc_trans=True)  # clean streams first: the reused buffers hold data
    assert first["status"].tolist() == [0, 0] and all(a[l["used"]] == 2 and a[l["skipped"]] == 0 for a, l in zip(first["acc"], lay))
    sym, offs = hmm._pack(clean + bad)
    got = hmm.loop_estep(models, sym, offs, lt, acc_trans=True)
    assert got["status"].tolist() == [0, 0, 1, 2, 1, 2, 1, 2]
    assert (got["log_prob"][2:] == NINF).all() and np.isfinite(got["log_prob"][:2]).all()
    for a, b, l in zip(got["acc"], first["acc"], lay):
        assert a[l["used"]] == 2 and a[l["skipped"]] == 6 and np.array_equal(a[:l["used"]], b[:l["used"]]) and a[:l["used"]].any()
    assert got["acc_trans"][-2:].tolist() == [2, 6] and np.array_equal(got["acc_trans"][:-2], first["acc_trans"][:-2])
    _assert_equal(got, R.estep(models, sym, offs, lt, acc_trans=True))
    only_bad = hmm.loop_estep(models, *hmm._pack(bad), lt, acc_trans=True)
    for a, l in zip(only_bad["acc"], lay):
        assert not a[:l["used"]].any() and a[l["used"]] == 0 and a[l["skipped"]] == 6
    assert not only_bad["acc_trans"][:-2].any()


@pytest.mark.parametrize("name", ["5x13", "21_22_64", "64x16"])
def test_one_call_a_call_per_stream_both_routes_and_chunk_budgets_give_the_same_limbs(name, monkeypatch):
    Ns = SETS[name]
    K, M = len(Ns), 32
    models = _init_models(Ns, M, 0, seed=77)
    rng = np.random.default_rng(4)
    streams = _streams(rng, M, list(range(0, 198, 18)) + [199, 100])  # 13 streams of 0 .. 199 frames
    sym, offs = hmm._pack(streams)
    lt = _matrix("random", K, 2)
    one = hmm.loop_estep(models, sym, offs, lt, acc_trans=True)
    _assert_equal(one, R.estep(models, sym, offs, lt, acc_trans=True))
    # a call per stream, summed on the host (AD is a sum of sums); the grammar table is added to and never cleared
    acc = [np.zeros_like(a) for a in one["acc"]]
    acc_t = np.zeros(hmm.transitions_acc_words(K), dtype=np.int64)
    for s in streams:
        r = hmm.loop_estep(models, s, [0, len(s)], lt, acc_trans=acc_t)
        assert r["acc_trans"] is acc_t
        for a, b in zip(acc, r["acc"]):
            a += b
    _assert_equal(dict(acc=acc, acc_trans=acc_t), one, keys=("acc", "acc_trans"))
    fits = name != "64x16"  # 16 sum N (N | 1) bytes of AN: 1 MiB there
    for var in ("ECOZ2_HMM_LOOP_EM_AN", "ECOZ2_HMM_LOOP_EM_C"):
        for route in ("global", "lds"):
            monkeypatch.setenv(var, route)
            if route == "lds" and var.endswith("AN") and not fits:
                with pytest.raises(e.Ecoz2Error) as ei:
                    hmm.loop_estep(models, sym, offs, lt, acc_trans=True)
                assert "bytes of LDS" in str(ei.value)
            else:
                _assert_equal(hmm.loop_estep(models, sym, offs, lt, acc_trans=True), one, (var, route))
        monkeypatch.delenv(var)
    slots = R.packing(Ns)[2]
    for budget in ("1", str(8 * (sum(Ns) + slots + K) * 500)):  # one stream per launch; a few streams per launch (a0 != 0)
        monkeypatch.setenv("ECOZ2_HMM_POSTERIOR_CHUNK_BYTES", budget)
        _assert_equal(hmm.loop_estep(models, sym, offs, lt, acc_trans=True), one, budget)


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
got = hmm.loop_estep(models, dev, d["offs"], d["lt"], acc_trans=True)
np.savez(sys.argv[3], acc=np.concatenate(got["acc"]), acc_trans=got["acc_trans"], log_prob=got["log_prob"], status=got["status"])
print("ok")
"""


def test_symbols_in_a_device_tensor(tmp_path):
    models = _init_models([5, 5, 5], 64, 0, seed=3)
    streams = _streams(np.random.default_rng(9), 64, (200, 0, 90))
    sym, offs = hmm._pack(streams)
    lt = _matrix("random", 3, 5)
    ref = hmm.loop_estep(models, sym, offs, lt, acc_trans=True)
    _assert_equal(ref, R.estep(models, sym, offs, lt, acc_trans=True))
    np.savez(tmp_path / "in.npz", pi=np.stack([m[0] for m in models]), A=np.stack([m[1] for m in models]),
             B=np.stack([m[2] for m in models]), sym=sym, offs=offs, lt=lt)
    r = subprocess.run([sys.executable, "-c", _TORCH_SCRIPT, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
    out = np.load(tmp_path / "out.npz")
    assert np.array_equal(out["acc"], np.concatenate(ref["acc"]))
    _assert_equal(out, ref, keys=("acc_trans", "log_prob", "status"))


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


def _models_equal(got, want, note=None):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(("pi", "A", "B"), g, w):
            assert np.array_equal(_bits(a), _bits(b)), (note, k, name)


@pytest.mark.parametrize("case", ["models", "matrix", "frozen"])
def test_three_iterations_of_the_training_equal_the_restatements_loop(case):
    models, streams = _corpus()
    sym, offs = hmm._pack(streams)
    start = np.log(np.array([[0.2, 0.5, 0.3], [0.3, 0.3, 0.4], [0.6, 0.1, 0.3]]))
    start[1, 0] = NINF  # a forbidden succession: it stays forbidden
    kw = dict(ln_switch=-1.5, val_auto=1e-6, max_iterations=3, epsilon=1e-5)
    if case == "models":
        kw.update(ln_p=None)
    elif case == "matrix":
        kw.update(ln_p=start, train_transitions=True, alpha=0.5)
    else:
        kw.update(ln_p=start, train_transitions=True, alpha=0.0, frozen=[0, 1, 0])
    seen = []
    got, got_p, hist = hmm.train_loop(models, sym, offs, callback=lambda v, x: seen.append((v, x)), **kw)
    want, want_p, whist = R.train(models, sym, offs, **kw)
    assert len(hist) == len(whist) == 3 and np.array_equal(_bits(hist), _bits(np.array(whist)))
    _models_equal(got, want, case)
    assert np.array_equal(_bits(got_p), _bits(want_p)), (got_p, want_p)
    assert seen == [("sum_log_prob", v) for v in whist]
    if case == "models":
        assert not got_p.any()  # the matrix is not written
    else:
        assert got_p[1, 0] == NINF and not np.array_equal(got_p, start)
    if case == "frozen":
        _models_equal(got[1:2], models[1:2], "the frozen class keeps every byte")
        assert not np.array_equal(got[0][2], models[0][2])
    # no stream of status 0: the call fails and names it
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.train_loop(models, np.array([16, 3], dtype=np.uint16), [0, 2], start, ln_switch=-1.5)
    assert "no stream can be explained" in str(ei.value)


def test_seventeen_slots_are_refused():
    models = _init_models([64] * 17, 4, 1)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.loop_estep(models, np.zeros(8, np.uint16), [0, 8], np.zeros((17, 17)))
    assert "17 wave-slots" in str(ei.value) and "e2vq_hmm_loop_estep" in str(ei.value)


# ---- files -----------------------------------------------------------------------------------------------------------------
def test_the_file_form_equals_the_array_calls_and_its_files_are_read_by_segment(tmp_path):
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

    # (the matrix starts from a file of distributions: from the default, a matrix of zeros, the first M-step takes two thirds of
    # the switching mass away and the sum of ln P may fall there)
    start = np.log(np.array([[0.2, 0.5, 0.3], [0.3, 0.3, 0.4], [0.6, 0.1, 0.3]]))
    hmm.write_class_transitions(tmp_path / "start.csv", names, start)
    out, err = run("hmm", "learn", "--loop", "-m", "hmms", "--switch-penalty", str(ls), "--class-transitions", "start.csv",
                   "--train-transitions", "--alpha", "0.5", "--freeze", "ship", "-a", "1e-6", "-I", "3", "-o", "out", "--sequences", *seqs)
    assert "3 E-step(s); 3 model(s) saved in out, out/transitions.csv saved; out/loop.csv saved" in out and err == ""
    sym, offs = hmm._pack(streams)
    want, want_p, hist = hmm.train_loop(models, sym, offs, hmm.read_class_transitions(tmp_path / "start.csv", names), ln_switch=ls,
                                        train_transitions=True, frozen=[0, 1, 0], alpha=0.5, val_auto=1e-6, max_iterations=3)
    assert len(hist) == 3
    got = [hmm.load_model(tmp_path / "out" / f"{c}.hmm")[1:] for c in names]
    _models_equal(got, want)
    assert np.array_equal(_bits(hmm.read_class_transitions(tmp_path / "out" / "transitions.csv", names)), _bits(want_p))
    g = lambda v: "%.17g" % v
    assert (tmp_path / "out" / "loop.csv").read_text() == "iteration,sum_log_prob,streams_used,streams_skipped\n" + "".join(
        f"{i},{g(v)},3,0\n" for i, v in enumerate(hist))
    # the Python mirror of the file call, from the matrix just written, without training it: no transitions.csv
    files = [str(tmp_path / "hmms" / f"{c}.hmm") for c in names]
    hmm.learn_loop_files(files, [str(tmp_path / s) for s in seqs], tmp_path / "out2", ls, class_transitions=tmp_path / "out" / "transitions.csv",
                         val_auto=1e-6, max_iterations=2)
    want2, _p, _h = hmm.train_loop(models, sym, offs, want_p, ln_switch=ls, val_auto=1e-6, max_iterations=2)
    _models_equal([hmm.load_model(tmp_path / "out2" / f"{c}.hmm")[1:] for c in names], want2)
    assert not (tmp_path / "out2" / "transitions.csv").exists() and (tmp_path / "out2" / "loop.csv").exists()
    # `hmm segment --class-transitions` reads the models and the matrix as they are
    run("hmm", "segment", "--models", "out", "--switch-penalty", str(ls), "--sequences", seqs[0], "--class-transitions", "out/transitions.csv",
        "-c", "seg")
    rows = (tmp_path / "seg" / "s0.csv").read_text().split("\n")
    assert len(rows) > 4 and rows[-1] == ""
