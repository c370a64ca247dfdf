"""`vq quantize --codebooks` without a device: what e2vq_vq_quantize_codebooks and e2vq_cbset_create refuse
before the first HIP call, the CLI's option handling, and the ISA properties k_quantize_set's rate rests on -- no scratch,
no spilled register, two waves per SIMD, and k_pass_mfma's tile loop (the P = 36 instantiation compiled for gfx950)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import vq
from tests.test_isa_guards import HIPCC, Kernel, compile_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
P = 12


def _cbook(path, M, order=P, seed=1):
    rng = np.random.default_rng(seed + M)
    refl = rng.uniform(-0.5, 0.5, (M, order + 1))
    refl[:, 0] = 1.0
    e.formats.write_cbook(str(path), "_", refl)
    return str(path)


def _prd(path, T=5, order=P, seed=3):
    e.formats.write_prd(str(path), "A", e.synth.synth_frames(seed, 4, order, 0, T))
    return str(path)


def _call(cbs, prds):
    c, _k1 = vq._to_vec_of_ptr_const_c_char(cbs)
    f, _k2 = vq._to_vec_of_ptr_const_c_char(prds)
    rc = e.lib.e2vq_vq_quantize_codebooks(c, len(cbs), f, len(prds), 0)
    return rc, e.lib.e2vq_last_error().decode(errors="replace")


@pytest.fixture
def out_root(tmp_path, monkeypatch):
    d = tmp_path / "out"
    d.mkdir()
    monkeypatch.setenv("ECOZ2_VQ_OUT_ROOT", str(d))
    return d


def _nothing_written(out_root):
    return [p for p in out_root.rglob("*")] == []


def test_refuses_empty_and_oversized_codebook_lists(tmp_path, out_root):
    prd = _prd(tmp_path / "a.prd")
    rc, msg = _call([], [prd])
    assert rc == 1 and "no codebooks" in msg
    # (the count is checked before any file is opened: these do not exist)
    rc, msg = _call([str(tmp_path / f"{k}.cbook") for k in range(65)], [prd])
    assert rc == 1 and "65 codebooks" in msg and "64" in msg
    assert _nothing_written(out_root)


def test_refuses_unreadable_files(tmp_path, out_root):
    cb, prd = _cbook(tmp_path / "m4.cbook", 4), _prd(tmp_path / "a.prd")
    missing_cb, missing_prd = str(tmp_path / "missing.cbook"), str(tmp_path / "missing.prd")
    rc, msg = _call([cb, missing_cb], [prd])
    assert rc == 1 and missing_cb in msg
    rc, msg = _call([cb], [prd, missing_prd])
    assert rc == 1 and missing_prd in msg
    assert _nothing_written(out_root)


def test_refuses_codebooks_of_differing_order(tmp_path, out_root):
    a, b = _cbook(tmp_path / "p12.cbook", 4), _cbook(tmp_path / "p16.cbook", 8, order=16)
    rc, msg = _call([a, b], [_prd(tmp_path / "a.prd")])
    assert rc == 1 and b in msg and "prediction order 16" in msg
    assert _nothing_written(out_root)


def test_refuses_two_codebooks_of_one_size(tmp_path, out_root):
    a, b, c = _cbook(tmp_path / "a.cbook", 4), _cbook(tmp_path / "b.cbook", 8), _cbook(tmp_path / "c.cbook", 4, seed=9)
    rc, msg = _call([a, b, c], [_prd(tmp_path / "a.prd")])
    assert rc == 1 and a in msg and c in msg and "M=4" in msg
    assert _nothing_written(out_root)


def test_refuses_a_predictor_file_of_another_order(tmp_path, out_root):
    cbs = [_cbook(tmp_path / "a.cbook", 4), _cbook(tmp_path / "b.cbook", 8)]
    # (the long file in front would get its .tmp files first if the plan ran before every header is read)
    long_one = _prd(tmp_path / "long.prd", T=3000)
    other = _prd(tmp_path / "p16.prd", order=16)
    os.environ["ECOZ2_VQ_QUANTIZE_CHUNK"] = "1024"
    try:
        rc, msg = _call(cbs, [long_one, other])
    finally:
        del os.environ["ECOZ2_VQ_QUANTIZE_CHUNK"]
    assert rc == 1 and other in msg and "prediction order 16" in msg
    assert _nothing_written(out_root)


@pytest.mark.parametrize("order,K,Ms,null_at,needle", [
    (P, 0, [], None, "0 codebooks"),
    (P, 65, [2] * 65, None, "65 codebooks"),
    (P, 2, [4, 0], None, "size 0"),
    (P, 2, [4, 65537], None, "size 65537"),
    (0, 1, [4], None, "prediction order 0"),
    (201, 1, [4], None, "prediction order 201"),
    (P, 2, [4, 8], 1, "codebook 1"),
])
def test_cbset_create_refuses_before_the_device(order, K, Ms, null_at, needle):
    keep = [np.zeros((max(m, 1), order + 1)) for m in Ms]
    ms = (C.c_int * max(K, 1))(*Ms)
    ptrs = (C.c_void_p * max(K, 1))(*[None if k == null_at else a.ctypes.data for k, a in enumerate(keep)])
    h = C.c_void_p(1)
    # device 1 << 20 does not exist anywhere: an argument check that came after the device check would name the device
    assert e.lib.e2vq_cbset_create(1 << 20, order, K, ms, ptrs, C.byref(h)) == 1
    msg = e.lib.e2vq_last_error().decode()
    assert needle in msg and "device" not in msg, msg
    assert not h.value


def test_cli_refuses_codebook_together_with_codebooks(tmp_path):
    cb, prd = _cbook(tmp_path / "a.cbook", 4), _prd(tmp_path / "a.prd")
    r = subprocess.run([CLI, "vq", "quantize", "--codebook", cb, "--codebooks", cb, "--predictors", prd], capture_output=True,
                       text=True, cwd=tmp_path)
    assert r.returncode != 0 and "usage:" in r.stderr and "vq quantize --codebooks" in r.stderr
    assert "nom_raas" not in r.stdout


def test_cli_expands_a_codebook_directory_sorted(tmp_path):
    d = tmp_path / "cbs"
    d.mkdir()
    names = ["eps_0.05_M_0008.cbook", "eps_0.05_M_0002.cbook", "eps_0.05_M_0004.cbook"]
    for n in names:
        _cbook(d / n, int(n[-10:-6]))
    (d / "notes.txt").write_text("not a codebook")
    extra = _cbook(tmp_path / "z16.cbook", 16)
    prd = _prd(tmp_path / "a.prd")
    env = dict(os.environ, ECOZ2_VQ_OUT_ROOT=str(tmp_path / "out"))
    r = subprocess.run([CLI, "vq", "quantize", "--codebooks", extra, str(d), "--predictors", prd], capture_output=True, text=True,
                       cwd=tmp_path, env=env)
    assert r.returncode == 0, r.stderr
    got = [l.split(" = ", 1)[1] for l in r.stdout.splitlines() if l.startswith("nom_raas = ")]
    # (the resolved list is sorted as a whole, path component by component, as for `vq classify --codebooks`)
    assert got == [str(d / n) for n in sorted(names)] + [extra]


# ---- ISA guard ---------------------------------------------------------------------------------------------------------------
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    return compile_asm("vq_device.hip", str(tmp_path_factory.mktemp("isa_set") / "vq_device.s"))


def _tile_loop(k):
    """the innermost loop that holds MFMAs: (MFMAs, full vector-memory waits)"""
    first, last, mfmas, waits = min((lp for lp in k.loops() if lp[2] > 0), key=lambda lp: lp[1] - lp[0])
    return mfmas, waits


@needs_hipcc
def test_quantize_set_kernel_isa(device_asm):
    k = Kernel(device_asm, r"k_quantize_setILi37E")
    # no scratch, no spilled VGPR, 512 / 2 registers: two waves per SIMD as __launch_bounds__(256, 2) assumes
    assert k.violations(256) == []
    assert k.count("scratch_") == 0
    # the tile loop is k_pass_mfma's (the row-major assignment sweep, MODE 0 / SRC 1): the same FP64 MFMAs in the kernel
    # and in its innermost loop
    ref = Kernel(device_asm, r"k_pass_mfmaILi37ELi0ELi256ELi1E")
    assert k.count("v_mfma_f64_16x16x4") == ref.count("v_mfma_f64_16x16x4") > 0
    assert _tile_loop(k)[0] == _tile_loop(ref)[0] > 0
