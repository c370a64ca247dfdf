"""`vq learn --all-classes`, CPU side: the argument checks of e2vq_vq_learn_classes /
e2vq_vq_train_classes run before any HIP call (so they answer the same with or without a device) and write no file; the
CLI refuses --all-classes with --class-name or -B; the class-batched kernels are in the gfx950 build without scratch or
spilled registers, and at every order class of the sweep no worse than the single-set sweep.  The GPU parity tests are in
test_gpu_vq_learn_classes.py and test_gpu_vq_learn_classes_shapes.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import vq
from ecoz2rs_amd._lib import LEARN_CALLBACK, LevelStatsC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
CLI = os.path.join(CSRC, "ecoz2")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
P = 12


def _err():
    return e.lib.e2vq_last_error().decode()


def _learn(files, P=P):
    f, _keep = vq._to_vec_of_ptr_const_c_char(files)
    return e.lib.e2vq_vq_learn_classes(P, 0.05, f, len(files), None, LEARN_CALLBACK(lambda *_a: None))


@pytest.fixture
def corpus(tmp_path, monkeypatch):
    monkeypatch.setenv("ECOZ2_VQ_OUT_ROOT", str(tmp_path / "out"))
    files = []
    for i, c in enumerate(("B", "A")):
        for k in range(2):
            p = tmp_path / "prd" / c / f"{k}.prd"
            p.parent.mkdir(parents=True, exist_ok=True)
            e.formats.write_prd(str(p), c, e.synth.synth_frames(5, 3, P, 100 * (2 * i + k), 50))
            files.append(str(p))
    return tmp_path, files


def _no_output(tmp_path):
    return not (tmp_path / "out").exists() or not any((tmp_path / "out").rglob("*"))


def _sparse_prd(path, T, P_):
    """a .prd whose header announces T frames of order P_, its payload a hole (no disk blocks)"""
    e.formats.write_prd(str(path), "S", np.zeros((1, P_ + 1)))
    with open(path, "r+b") as f:
        f.seek(0)
        head = bytearray(f.read(120))
        head[112:116] = int(T).to_bytes(4, "little")
        f.seek(0)
        f.write(bytes(head))
        f.truncate(120 + T * (P_ + 1) * 8)


@pytest.mark.parametrize("case,needle", [
    ("empty", "no predictor files"),
    ("unreadable", "missing.prd"),
    ("order", "prediction order 12, expected 16"),
    ("order_mixed", "prediction order 16, expected 12"),
    ("empty_class", "class 'Z' has no training vectors"),
    ("order_range", "prediction order 0 out of range"),
])
def test_learn_classes_refuses_before_the_device(corpus, case, needle):
    tmp_path, files = corpus
    if case == "empty":
        rc = _learn([])
    elif case == "unreadable":
        rc = _learn(files + [str(tmp_path / "missing.prd")])
    elif case == "order":
        rc = _learn(files, P=16)
    elif case == "order_mixed":
        p = tmp_path / "prd" / "C" / "p16.prd"
        p.parent.mkdir(parents=True, exist_ok=True)
        e.formats.write_prd(str(p), "C", e.synth.synth_frames(5, 3, 16, 0, 10))
        rc = _learn(files + [str(p)])
    elif case == "empty_class":
        p = tmp_path / "prd" / "Z" / "none.prd"
        p.parent.mkdir(parents=True, exist_ok=True)
        e.formats.write_prd(str(p), "Z", np.zeros((0, P + 1)))
        rc = _learn(files + [str(p)])
    else:
        rc = _learn(files, P=0)
    assert rc == 1 and needle in _err(), _err()
    assert _no_output(tmp_path)


def test_learn_classes_refuses_more_than_the_frame_bound(tmp_path, monkeypatch):
    monkeypatch.setenv("ECOZ2_VQ_OUT_ROOT", str(tmp_path / "out"))
    big = tmp_path / "big.prd"
    _sparse_prd(big, 1 << 26, 1)
    rc = _learn([str(big)] * 32, P=1)  # 2^31 frames
    assert rc == 1 and "exceed the limit of 2^31 - 65" in _err(), _err()
    assert _no_output(tmp_path)


def _train_rc(P_=P, K=None, class_offs=(0, 3, 5), max_M=4, frames_T=None):
    K = len(class_offs) - 1 if K is None else K
    co = np.array(class_offs, dtype=np.int64)
    T = int(frames_T if frames_T is not None else max(int(co[-1]), 1))
    frames = np.ones((T, P_ + 1))
    cbs = np.zeros((max(K, 1), max(max_M, 1), P_ + 1))
    levels = (LevelStatsC * (max(K, 1) * 4))()
    n = np.zeros(max(K, 1), dtype=np.int32)
    return e.lib.e2vq_vq_train_classes(0, P_, K, frames.ctypes.data, co.ctypes.data, 0.05, max_M, cbs.ctypes.data, levels, 4,
                                       n.ctypes.data)


@pytest.mark.parametrize("kw,needle", [
    (dict(class_offs=(0, 2, 2, 4)), "not strictly increasing at class 1"),
    (dict(class_offs=(0, 3, 1, 4)), "not strictly increasing at class 1"),
    (dict(class_offs=(1, 2, 4)), "class_offs must start at 0"),
    (dict(class_offs=(0,), K=0), "bad arguments (K = 0)"),
    (dict(max_M=6), "max_M = 6: expected a power of two"),
    (dict(max_M=0), "max_M = 0: expected a power of two"),
    (dict(P_=0), "prediction order 0 out of range"),
    (dict(class_offs=(0, 5, 1 << 31), frames_T=8), "exceed the limit of 2^31 - 65"),
])
def test_train_classes_refuses_before_the_device(kw, needle):
    assert _train_rc(**kw) == 1
    assert needle in _err(), _err()


def test_python_train_codebooks_refuses_an_empty_class():
    with pytest.raises(RuntimeError, match="not strictly increasing"):
        vq.train_codebooks([np.ones((3, P + 1)), np.zeros((0, P + 1))], P, 0.05, 4)


def test_python_learn_classes_refuses_an_empty_list():
    with pytest.raises(RuntimeError, match="no predictor files"):
        vq.vq_learn_classes(P, 0.05, [])


# ---- CLI ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--class-name", "A"], ["-B", "x.cbook"]])
def test_cli_all_classes_excludes_class_name_and_base(corpus, extra):
    tmp_path, files = corpus
    r = subprocess.run([CLI, "vq", "learn", "--all-classes", "-P", str(P), *extra, "--predictors", *files], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2, r
    assert "--all-classes excludes --class-name and -B" in r.stderr
    assert "vq learn --all-classes" in r.stderr  # (the usage text names the form)
    assert _no_output(tmp_path)


# ---- ISA guard (style of test_isa_guards.py) ---------------------------------------------------------------------------
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip", "--cuda-device-only", "-S",
         "-DE2VQ_PRE_NC_LIST(X)=X(37)", "-DE2VQ_MFMA_NC_LIST(X)=X(37)", "-DE2VQ_MFMA_WIDE_NC_LIST(X)=X(49)"]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    d = tmp_path_factory.mktemp("isa")
    out = {}
    for name in ("vq_device", "vq_update"):
        path = str(d / (name + ".s"))
        subprocess.run([HIPCC, *FLAGS, "-o", path, os.path.join(CSRC, name + ".hip")], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL, timeout=900)
        out[name] = open(path).read()
    return out


def _metas(text):
    res = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", m.group(2)).group(1))
        res[m.group(1)] = dict(vgpr=g("vgpr_count"), spill=g("vgpr_spill_count"), scratch=g("private_segment_fixed_size"))
    return res


def _one(metas, pattern):
    hits = [n for n in metas if re.search(pattern, n)]
    assert len(hits) == 1, f"{pattern}: {hits}"
    return metas[hits[0]]


CLASS_KERNELS = [("vq_device", r"k_pass_mfma_classesILi37ELi1ELi512E"), ("vq_device", r"k_pass_mfma_classesILi37ELi5ELi512E"),
                 ("vq_device", r"k_pass_mfma_classesILi37ELi2ELi512E"), ("vq_device", r"k_pass_mfma_classesILi49ELi2ELi512E"),
                 ("vq_update", r"k_zero_rows_classes"), ("vq_update", r"k_rows_stats_classes"),
                 ("vq_update", r"k_centroids_classes"), ("vq_update", r"k_level_record_classes"),
                 ("vq_update", r"k_codebook_prepare_classes"), ("vq_update", r"k_grow_classes")]


@pytest.mark.parametrize("src,kernel", CLASS_KERNELS)
def test_batched_kernels_have_no_scratch_and_no_spill(asm, src, kernel):
    m = _one(_metas(asm[src]), kernel)
    assert m["scratch"] == 0 and m["spill"] == 0, m


def _waves_per_simd(vgpr):
    """gfx950: 512 unified registers per SIMD lane, allocated in granules of 8"""
    return 512 // ((vgpr + 7) // 8 * 8)


@pytest.mark.parametrize("nc,mode", [(37, 1), (37, 5), (37, 2), (49, 2)])
def test_batched_sweep_keeps_the_single_set_register_budget(asm, nc, mode):
    """k_pass_mfma_classes runs k_pass_mfma's body from a table entry: it stays within the budget of the launch bounds both
    declare (two waves per SIMD) and keeps the single-set kernel's occupancy; at most a few registers more (the scheduler
    spends what the occupancy leaves free differently: DESIGN.md 4.9.1)"""
    metas = _metas(asm["vq_device"])
    batched = _one(metas, rf"k_pass_mfma_classesILi{nc}ELi{mode}ELi512E")
    single = _one(metas, rf"11k_pass_mfmaILi{nc}ELi{mode}ELi512ELi0E")
    assert batched["vgpr"] <= 256 and _waves_per_simd(batched["vgpr"]) == _waves_per_simd(single["vgpr"]) == 2, (batched, single)
    assert batched["vgpr"] <= single["vgpr"] + 8, (batched, single)


# every order class of the sweep: NC = 5 (REM 1, the trailing VALU fma), 8 (REM 4), 41 (the last narrow order), 42 and 81 (the
# first and the last wide order)
WIDE_FLAGS = [f for f in FLAGS if not f.startswith("-DE2VQ_")] + [
    "-DE2VQ_PRE_NC_LIST(X)=X(41)", "-DE2VQ_MFMA_NC_LIST(X)=X(5) X(8) X(41)", "-DE2VQ_MFMA_WIDE_NC_LIST(X)=X(42) X(81)"]
ORDER_CLASSES = [(5, 1), (5, 5), (5, 2), (8, 1), (8, 5), (8, 2), (41, 1), (41, 5), (41, 2), (42, 2), (81, 2)]


@pytest.fixture(scope="module")
def asm_orders(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    path = str(tmp_path_factory.mktemp("isa_orders") / "vq_device.s")
    subprocess.run([HIPCC, *WIDE_FLAGS, "-o", path, os.path.join(CSRC, "vq_device.hip")], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=900)
    return _metas(open(path).read())


def test_order_classes_are_all_instantiated(asm_orders):
    got = {tuple(int(x) for x in m.groups()) for n in asm_orders for m in [re.search(r"k_pass_mfma_classesILi(\d+)ELi(\d+)ELi512E", n)]
           if m}
    assert got == set(ORDER_CLASSES)


@pytest.mark.parametrize("nc,mode", ORDER_CLASSES)
def test_batched_sweep_is_no_worse_than_the_single_set_sweep(asm_orders, nc, mode):
    """k_pass_mfma_classes<NC, MODE> against k_pass_mfma<NC, MODE, 512, 0> at every order class: the same occupancy, no more
    spilled registers, no more scratch.  At NC = 41 mode 1 (P = 40, M <= 128) both spill today -- the largest narrow order
    fills the 256 registers of two waves per SIMD with four frame tiles of 11 k-steps plus the prefetched next block -- so
    the batched kernel is held to the single-set kernel's figures there and to none elsewhere."""
    batched = _one(asm_orders, rf"k_pass_mfma_classesILi{nc}ELi{mode}ELi512E")
    single = _one(asm_orders, rf"11k_pass_mfmaILi{nc}ELi{mode}ELi512ELi0E")
    assert batched["vgpr"] <= 256 and _waves_per_simd(batched["vgpr"]) == _waves_per_simd(single["vgpr"]), (batched, single)
    assert batched["spill"] <= single["spill"] and batched["scratch"] <= single["scratch"], (batched, single)
    if (nc, mode) != (41, 1):
        assert batched["scratch"] == 0 and batched["spill"] == 0, batched
