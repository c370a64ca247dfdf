"""`hmm learn --all-classes`, CPU side: the argument checks of e2vq_hmm_learn_classes /
e2vq_hmm_train_classes run before any HIP call (so they answer the same with or without a device) and write no file.
The classes train as the one-(N, M) case of the grid batch, whose kernels test_hmm_learn_grid_cpu.py guards.  The GPU
parity tests are in test_gpu_hmm_learn_classes.py."""
import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm


def _err():
    return e.lib.e2vq_last_error().decode()


def _learn(files, N=5, typ=3):
    f, _keep = hmm._strs(files)
    return e.lib.e2vq_hmm_learn_classes(N, typ, f, len(files), 1e-5, 0.3, -1, hmm.HMM_LEARN_CALLBACK(lambda v, x: None))


@pytest.fixture
def corpus(tmp_path, monkeypatch):
    monkeypatch.setenv("ECOZ2_VQ_OUT_ROOT", str(tmp_path / "out"))
    rng = np.random.default_rng(3)
    files = []
    for c in ("B", "A"):
        for k in range(3):
            p = tmp_path / "seq" / c / f"{k}.seq"
            p.parent.mkdir(parents=True, exist_ok=True)
            e.formats.write_seq(str(p), c, 16, rng.integers(0, 16, 20))
            files.append(str(p))
    return tmp_path, files


def _no_output(tmp_path):
    return not (tmp_path / "out").exists() or not any((tmp_path / "out").rglob("*"))


@pytest.mark.parametrize("case,needle", [
    ("empty", "no sequences"),
    ("N0", "number of states 0 not in [1, 512]"),
    ("N513", "number of states 513 not in [1, 512]"),
    ("type", "model type 4 not in 0..3"),
    ("typeneg", "model type -1 not in 0..3"),
    ("mixed_M", "codebook size 32 differs"),
    ("symbol", "symbol 16 outside the codebook size 16"),
])
def test_learn_classes_refuses_before_the_device(corpus, case, needle):
    tmp_path, files = corpus
    if case == "empty":
        rc = _learn([])
    elif case == "N0":
        rc = _learn(files, N=0)
    elif case == "N513":
        rc = _learn(files, N=513)
    elif case == "type":
        rc = _learn(files, typ=4)
    elif case == "typeneg":
        rc = _learn(files, typ=-1)
    elif case == "mixed_M":
        p = tmp_path / "seq" / "C" / "m32.seq"
        p.parent.mkdir(parents=True, exist_ok=True)
        e.formats.write_seq(str(p), "C", 32, np.arange(10))
        rc = _learn(files + [str(p)])
    else:
        p = tmp_path / "seq" / "A" / "bad.seq"
        e.formats.write_seq(str(p), "A", 16, [1, 2, 16, 3])
        rc = _learn(files + [str(p)])
    assert rc == 1 and needle in _err(), _err()
    assert _no_output(tmp_path)


def _train_classes_rc(N=3, M=8, class_offs=(0, 2, 4), S=4, K=None):
    K = len(class_offs) - 1 if K is None else K
    pi, A, B = np.full((K, max(N, 1)), 0.5), np.full((K, max(N, 1), max(N, 1)), 0.5), np.full((K, max(N, 1), max(M, 1)), 0.5)
    sym = np.zeros(4 * S, dtype=np.uint16)
    offs = np.arange(S + 1, dtype=np.int64) * 4
    co = np.array(class_offs, dtype=np.int64)
    hist, n = np.zeros((K, 8)), np.zeros(K, dtype=np.int32)
    return e.lib.e2vq_hmm_train_classes(0, N, M, K, pi.ctypes.data, A.ctypes.data, B.ctypes.data, sym.ctypes.data,
                                        offs.ctypes.data, S, co.ctypes.data, 1e-5, 0.3, -1, hist.ctypes.data, 8,
                                        n.ctypes.data)


@pytest.mark.parametrize("kw,needle", [
    (dict(class_offs=(0, 2, 2, 4)), "not strictly increasing at class 1"),
    (dict(class_offs=(0, 3, 1, 4)), "not strictly increasing at class 1"),
    (dict(class_offs=(1, 2, 4)), "from 0 to S = 4"),
    (dict(class_offs=(0, 2, 3)), "from 0 to S = 4"),
    (dict(N=0), "N=0 M=8 out of range"),
    (dict(N=513), "N=513 M=8 out of range"),
    (dict(M=0), "N=3 M=0 out of range"),
    (dict(class_offs=(0,), K=0), "bad arguments (K = 0)"),
])
def test_train_classes_refuses_before_the_device(kw, needle):
    assert _train_classes_rc(**kw) == 1
    assert needle in _err(), _err()


def test_python_train_classes_checks_the_class_count():
    with pytest.raises(ValueError):
        hmm.train_classes([(np.ones(2) / 2, np.ones((2, 2)) / 2, np.ones((2, 4)) / 4)], [[], []])
