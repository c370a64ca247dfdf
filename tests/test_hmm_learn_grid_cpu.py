"""`hmm learn --grid`, CPU side: the argument checks of e2vq_hmm_learn_grid / e2vq_hmm_train_grid and
of the CLI run before any HIP call (so they answer the same with or without a device) and write no file; `--all-classes`
without `--grid` still refuses mixed M; the grid kernels are in the gfx950 build without scratch or spilled registers.
The GPU parity tests are in test_gpu_hmm_learn_grid.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXE = os.path.join(CSRC, "ecoz2")


def _err():
    return e.lib.e2vq_last_error().decode()


def _learn_grid(files, Ns=(3, 5), typ=3):
    f, _keep = hmm._strs(files)
    ns = (hmm.C.c_int * max(len(Ns), 1))(*Ns)
    return e.lib.e2vq_hmm_learn_grid(ns, len(Ns), typ, f, len(files), 1e-5, 0.3, -1, hmm.HMM_LEARN_CALLBACK(lambda v, x: None))


@pytest.fixture
def corpus(tmp_path, monkeypatch):
    """classes A and B at M = 16, class A at M = 32"""
    monkeypatch.setenv("ECOZ2_VQ_OUT_ROOT", str(tmp_path / "out"))
    rng = np.random.default_rng(3)
    files = []
    for c, M in (("B", 16), ("A", 16), ("A", 32)):
        for k in range(3):
            p = tmp_path / "seq" / f"M{M}" / c / f"{k}.seq"
            p.parent.mkdir(parents=True, exist_ok=True)
            e.formats.write_seq(str(p), c, M, rng.integers(0, M, 20))
            files.append(str(p))
    return tmp_path, files


def _no_output(tmp_path):
    return not (tmp_path / "out").exists() or not any((tmp_path / "out").rglob("*"))


@pytest.mark.parametrize("case,needle", [
    ("empty", "e2vq_hmm_learn_grid: no sequences"),
    ("no_N", "e2vq_hmm_learn_grid: no number of states given"),
    ("dup_N", "number of states 5 given more than once"),
    ("N0", "number of states 0 not in [1, 512]"),
    ("N513", "number of states 513 not in [1, 512]"),
    ("type", "model type 4 not in 0..3"),
    ("typeneg", "model type -1 not in 0..3"),
    ("symbol", "symbol 16 outside the codebook size 16"),
])
def test_learn_grid_refuses_before_the_device(corpus, case, needle):
    tmp_path, files = corpus
    if case == "empty":
        rc = _learn_grid([])
    elif case == "no_N":
        rc = _learn_grid(files, Ns=())
    elif case == "dup_N":
        rc = _learn_grid(files, Ns=(5, 3, 5))
    elif case == "N0":
        rc = _learn_grid(files, Ns=(3, 0))
    elif case == "N513":
        rc = _learn_grid(files, Ns=(513, 4))
    elif case == "type":
        rc = _learn_grid(files, typ=4)
    elif case == "typeneg":
        rc = _learn_grid(files, typ=-1)
    else:  # (a symbol that the M = 32 files may hold, in a file of M = 16)
        p = tmp_path / "seq" / "M16" / "A" / "bad.seq"
        e.formats.write_seq(str(p), "A", 16, [1, 2, 16, 3])
        rc = _learn_grid(files + [str(p)])
    assert rc == 1 and needle in _err(), _err()
    assert _no_output(tmp_path)


def test_all_classes_still_refuses_mixed_M(corpus):
    tmp_path, files = corpus
    f, _keep = hmm._strs(files)
    rc = e.lib.e2vq_hmm_learn_classes(5, 3, f, len(files), 1e-5, 0.3, -1, hmm.HMM_LEARN_CALLBACK(lambda v, x: None))
    assert rc == 1 and "codebook size 32 differs" in _err(), _err()
    assert _no_output(tmp_path)


def _train_grid_rc(Ns=(3, 4), Ms=(8, 8), param_offs=None, ranges=((0, 2), (1, 4)), S=4, sym_max=0, K=None):
    K = len(Ns) if K is None else K
    sizes = [n + n * n + n * m for n, m in zip(Ns, Ms)]
    if param_offs is None:
        param_offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]) if sizes else []
    params = np.full(max(sum(max(s, 1) for s in sizes), 1) * 2, 0.5)
    sym = np.zeros(4 * S, dtype=np.uint16)
    sym[0] = sym_max
    offs = np.arange(S + 1, dtype=np.int64) * 4
    ns, ms = np.array(Ns, dtype=np.int32), np.array(Ms, dtype=np.int32)
    po = np.array(param_offs, dtype=np.int64)
    lo = np.array([r[0] for r in ranges], dtype=np.int64)
    hi = np.array([r[1] for r in ranges], dtype=np.int64)
    hist, n = np.zeros((max(K, 1), 8)), np.zeros(max(K, 1), dtype=np.int32)
    return e.lib.e2vq_hmm_train_grid(0, K, ns.ctypes.data, ms.ctypes.data, params.ctypes.data, po.ctypes.data, sym.ctypes.data,
                                     offs.ctypes.data, S, lo.ctypes.data, hi.ctypes.data, 1e-5, 0.3, -1, hist.ctypes.data, 8,
                                     n.ctypes.data)


@pytest.mark.parametrize("kw,needle", [
    (dict(K=0, Ns=(), Ms=(), ranges=()), "bad arguments (K = 0)"),
    (dict(Ns=(3, 0)), "model 1: HMM with N=0 M=8 out of range"),
    (dict(Ns=(513, 3)), "model 0: HMM with N=513 M=8 out of range"),
    (dict(Ms=(8, 0)), "model 1: HMM with N=4 M=0 out of range"),
    (dict(ranges=((0, 2), (2, 2))), "model 1: sequence range [2, 2) not a non-empty part of [0, 4)"),
    (dict(ranges=((3, 1), (0, 4))), "model 0: sequence range [3, 1) not a non-empty part of [0, 4)"),
    (dict(ranges=((-1, 2), (0, 4))), "model 0: sequence range [-1, 2) not a non-empty part of [0, 4)"),
    (dict(ranges=((0, 2), (1, 5))), "model 1: sequence range [1, 5) not a non-empty part of [0, 4)"),
    (dict(param_offs=(0, 10)), "parameter blocks overlap: [0, 36) and [10, 62)"),
    (dict(param_offs=(36, 0)), "parameter blocks overlap: [0, 52) and [36, 72)"),
    (dict(param_offs=(0, -1)), "model 1: parameter offset -1 < 0"),
    (dict(Ms=(8, 16), sym_max=8), "model 0: symbol 8 outside the codebook size 8"),
    (dict(Ms=(16, 8), ranges=((0, 4), (0, 4)), sym_max=8), "model 1: symbol 8 outside the codebook size 8"),
])
def test_train_grid_refuses_before_the_device(kw, needle):
    assert _train_grid_rc(**kw) == 1
    assert needle in _err(), _err()


def test_python_train_grid_checks_the_range_count():
    with pytest.raises(ValueError):
        hmm.train_grid([(np.ones(2) / 2, np.ones((2, 2)) / 2, np.ones((2, 4)) / 4)], [np.zeros(3, np.uint16)], [(0, 1), (0, 1)])


# ---- CLI ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def cli_tree(tmp_path):
    for M, classes in ((16, ("C0", "C1")), (33, ("C0",))):
        for c in classes:
            for k in range(2):
                p = tmp_path / "data" / "sequences" / f"M{M}" / c / f"{k:05d}.seq"
                p.parent.mkdir(parents=True, exist_ok=True)
                e.formats.write_seq(str(p), c, M, np.arange(12) % M)
    (tmp_path / "tt.csv").write_text("tt,class,selection\nTRAIN,C0,00000\nTRAIN,C0,00001\nTRAIN,C1,00000\n")
    return tmp_path


def _cli(root, *args):
    env = dict(os.environ, ECOZ2_VQ_OUT_ROOT=str(root / "out"))
    r = subprocess.run([EXE, "hmm", "learn", *args], cwd=root, env=env, capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("args,code,needle", [
    (["--grid", "--class-name", "C0", "-N", "3", "-M", "16", "--sequences", "tt.csv"], 2, "--grid and --class-name exclude each other"),
    (["--grid", "-N", "3,x", "-M", "16", "--sequences", "tt.csv"], 2, "comma-separated integers"),
    (["--grid", "-N", "3,5", "-M", "16,", "--sequences", "tt.csv"], 2, "comma-separated integers"),
    (["--grid", "-N", "3", "--sequences", "tt.csv"], 2, "comma-separated integers"),
    (["--grid", "-N", "3", "-M", "16,33,16", "--sequences", "tt.csv"], 2, "-M 16: given more than once"),
    (["--grid", "-N", "3", "-M", "0,16", "--sequences", "tt.csv"], 2, "-M 0: not a codebook size"),
    (["--grid", "-N", "3", "-M", "16", "--sequences", "data/sequences"], 0, "codebook size 33 is not in the -M list"),
    (["--grid", "-N", "3", "-M", "16,33,64", "--sequences", "data/sequences"], 0,
     "no sequence with codebook size 64 among the given ones"),
    (["--grid", "-N", "3,3", "-M", "16,33", "--sequences", "data/sequences"], 0, "number of states 3 given more than once"),
    (["--grid", "-N", "3,600", "-M", "16", "--sequences", "tt.csv"], 0, "number of states 600 not in [1, 512]"),
    (["--grid", "-N", "3", "-M", "16", "-t", "7", "--sequences", "tt.csv"], 0, "model type 7 not in 0..3"),
])
def test_cli_grid_refusals(cli_tree, args, code, needle):
    rc, out, err = _cli(cli_tree, *args)
    assert rc == code and needle in (err if code == 2 else out), (rc, out, err)
    assert not (cli_tree / "out").exists()


def test_cli_usage_names_the_grid(cli_tree):
    rc, _out, err = _cli(cli_tree, "--grid", "--class-name", "C0", "-M", "16", "--sequences", "tt.csv")
    assert rc == 2 and "ecoz2 hmm learn --grid -N <n1,n2,...> -M <m1,m2,...>" in err


def test_cli_all_classes_still_refuses_mixed_M(cli_tree):
    rc, out, err = _cli(cli_tree, "--all-classes", "-N", "3", "-M", "16", "--sequences", "data/sequences")
    assert rc == 0 and "differs from the first sequence's" in out, (out, err)
    assert not (cli_tree / "out").exists()


# ---- ISA guard (style of test_isa_guards.py) ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_device.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_device.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _meta(text, pattern):
    metas = [(m.group(1), m.group(2)) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S)
             if re.search(pattern, m.group(1))]
    assert len(metas) == 1, f"{pattern}: {[n for n, _ in metas]}"
    g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0][1]).group(1))
    return dict(vgpr=g("vgpr_count"), spill=g("vgpr_spill_count"), scratch=g("private_segment_fixed_size"))


@pytest.mark.parametrize("kernel", ["k_hmm_fb_grid", "k_hmm_reestimate_grid", "k_hmm_adjustb_grid"])
def test_grid_kernels_have_no_scratch_and_no_spill(asm, kernel):
    m = _meta(asm, kernel)
    assert m["scratch"] == 0 and m["spill"] == 0, m


def test_grid_estep_keeps_the_single_model_register_budget(asm):
    """the grid E-step runs k_hmm_fb's body: it must not need more registers (occupancy of the 4-wave groups)"""
    assert _meta(asm, r"k_hmm_fb_grid")["vgpr"] <= _meta(asm, r"8k_hmm_fbENS")["vgpr"]
