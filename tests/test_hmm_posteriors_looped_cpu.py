"""The looped body of `hmm segment --posteriors` (ECOZ2_HMM_POSTERIOR_BODY), CPU side: the restatement without
its cap of 16 slots against the contract in plain loops at 17 slots and against the capped one below; its rows summing to 1;
what the opt-in changes before any HIP call -- a bad word is refused from arrays, from files, by the Python mirror and by the
CLI, `--body` needs `--posteriors`, the 17-slot refusal keeps every word with nothing set and under `resident` and goes under
`auto` and `looped` --; the LDS formula against the source; the new kernels' compiler metadata; the exports.  The GPU parity
tests are in test_gpu_hmm_posteriors_looped.py."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_posterior_looped_cases as LC
from . import hmm_posterior_restatement as R
from .test_hmm_posteriors_cpu import _err, _posteriors_c, _uniform, tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXE = os.path.join(CSRC, "ecoz2")
NINF = float("-inf")
SLOTS17 = "the classes take 17 wave-slots of 64 lanes (at most 16: the posteriors have no looped body)"
BAD = "ECOZ2_HMM_POSTERIOR_BODY=fast: auto, resident or looped"


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in (LC.BODY, LC.CHUNK):
        monkeypatch.delenv(k, raising=False)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- the restatement above 16 slots ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, T", [("33x17", 5), ("5x193", 4)])
def test_the_uncapped_restatement_is_the_transcription_at_seventeen_slots(name, T):
    Ns, M = LC.WIDE[name]
    assert LC.slots_of(Ns) == 17
    models = LC.wide_models(name)
    seq = LC.loop_cases.run_stream(3, len(Ns), M, T, run=2)
    for ls in (NINF, -3.0, 0.0):
        got = LC.posteriors_one(models, seq, ls)
        post, lp, st = R.transcribe(models, seq, ls)
        assert got["status"] == st == 0 and _bits(got["log_prob"]) == _bits(lp)
        assert np.array_equal(_bits(got["post"]), _bits(np.array(post).reshape(T, len(Ns))))
    assert R.MAX_SLOTS == 16  # (the cap is lifted for the call only)
    with pytest.raises(AssertionError):
        R.posteriors_one(models, seq, -3.0)


@pytest.mark.parametrize("name", ["5x13", "21_22_64", "64x16"])
def test_the_uncapped_restatement_is_the_capped_one_up_to_sixteen_slots(name):
    Ns, M = LC.RESIDENT[name], 8
    models = LC.loop_cases.leaning_models(5, Ns, M)
    sym, offs = LC.pack(LC.streams(len(Ns), M, (0, 1, 9, 30), K=len(Ns)))
    for ls in (NINF, -3.0):
        got, want = LC.posteriors(models, sym, offs, ls), R.posteriors(models, sym, offs, ls)
        assert all(np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes() for k in ("post", "log_prob", "status"))


@pytest.mark.parametrize("name", list(LC.WIDE))
def test_the_rows_of_the_wide_references_sum_to_one(name):
    Ns, _M = LC.WIDE[name]
    models, sym, offs = LC.wide_case(name)
    assert LC.slots_of(Ns) > 16 and len(models) == len(Ns)
    want = LC.wide_reference(name, -3.0)
    assert want["status"].tolist() == [0] * len(LC.LENGTHS) and want["post"].min() >= 0.0
    err = float(np.max(np.abs(want["post"].sum(axis=1) - 1.0)))
    print(f"{name}: rows sum to 1 within {err:.3e}")
    assert err <= tolerance(max(LC.LENGTHS), max(Ns))


def test_the_wide_sets_are_what_their_comments_say():
    slots = {name: LC.slots_of(Ns) for name, (Ns, _M) in LC.WIDE.items()}
    assert slots == {"33x17": 17, "5x193": 17, "33x33": 33, "64x20": 20, "mixed": 18}
    a_lds = {name: LC.looped_route(Ns)["a_lds"] for name, (Ns, _M) in LC.WIDE.items()}
    assert a_lds == {"33x17": True, "5x193": True, "33x33": False, "64x20": False, "mixed": False}
    per_slot = np.bincount(LC.loop_cases.slot_of_class(LC.WIDE["mixed"][0]))
    assert (per_slot == 1).sum() == 11 and (per_slot > 1).sum() == 7 and LC.loop_cases.one_class_slot_next_to_packed(LC.WIDE["mixed"][0])
    assert [LC.looped_route(Ns)["a_lds"] for Ns in LC.RESIDENT.values()] == [True] * 8 + [False]


# ---- before the device -----------------------------------------------------------------------------------------------------------
def _files(tmp_path, n=17, N=33):
    d = tmp_path / "in"
    d.mkdir()
    models = []
    for k in range(n):
        hmm.save_model(d / f"c{k:02d}.hmm", f"c{k:02d}", *_uniform(N, 16))
        models.append(str(d / f"c{k:02d}.hmm"))
    e.formats.write_seq(str(d / "x.seq"), "A", 16, np.arange(40) % 16)
    return models, [str(d / "x.seq")]


def _files_c(models, inputs, csv=None):
    m, _k1 = hmm._strs(models)
    f, _k2 = hmm._strs(inputs)
    return e.lib.e2vq_hmm_segment_files_posteriors(m, len(models), None, f, len(inputs), 4, 45, 15, -5.0, str(csv).encode() if csv else None, None)


def test_a_bad_word_is_refused_from_arrays_from_files_by_the_mirror_and_by_the_cli(monkeypatch, tmp_path):
    models, inputs = _files(tmp_path, n=2, N=3)
    ok = [_uniform(3, 8)]
    with pytest.raises(e.Ecoz2Error):
        hmm.segment_posteriors(ok, np.zeros(8, np.uint16), [0, 8], -1.0, body="fast")
    assert _err() == BAD
    with pytest.raises(e.Ecoz2Error):
        hmm.segment_files(models, inputs, -5.0, csv=tmp_path / "o", posteriors=True, body="fast")
    assert _err() == BAD and not (tmp_path / "o").exists()
    assert LC.BODY not in os.environ  # (the wrappers restore the environment)
    with pytest.raises(ValueError):
        hmm.segment_files(models, inputs, -5.0, body="auto")
    monkeypatch.setenv(LC.BODY, "fast")
    assert _posteriors_c(ok, -1.0) == 1 and _err() == BAD
    assert _files_c(models, inputs, csv=tmp_path / "o") == 1 and _err() == BAD and not (tmp_path / "o").exists()
    # (the earlier checks keep their place: a bad price is seen before the variable)
    assert _posteriors_c(ok, 0.5) == 1 and "ln_switch = 0.5" in _err()
    monkeypatch.delenv(LC.BODY)
    common = ["hmm", "segment", "--models", "a.hmm", "--sequences", "x.seq", "--switch-penalty", "-5"]
    r = subprocess.run([EXE, *common, "--posteriors", "--body", "fast"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "hmm segment --posteriors: --body fast: auto, resident or looped" in r.stderr and "ecoz2 hmm segment" in r.stderr
    r = subprocess.run([EXE, *common, "--body", "auto"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "hmm segment: --body <auto|resident|looped> needs --posteriors" in r.stderr
    r = subprocess.run([EXE, *common, "--posteriors", "--body"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--body needs a value" in r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert "                  [--posteriors [--frame-posteriors <dir>]]\n                  [--body <auto|resident|looped>]\n" in r.stderr + r.stdout


@pytest.mark.parametrize("body", [None, "", "resident"])
def test_the_old_refusal_keeps_every_word_with_resident_and_with_nothing_set(monkeypatch, tmp_path, body):
    if body is not None:
        monkeypatch.setenv(LC.BODY, body)
    for models in ([_uniform(64, 8)] * 17, [_uniform(33, 8)] * 17):
        assert _posteriors_c(models, -1.0) == 1 and _err() == "e2vq_hmm_segment_posteriors: " + SLOTS17
    files, inputs = _files(tmp_path)
    assert _files_c(files, inputs) == 1 and _err() == "e2vq_hmm_segment_files_posteriors: " + SLOTS17
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment_posteriors([_uniform(64, 8)] * 17, np.zeros(8, np.uint16), [0, 8], -1.0, body="resident")
    assert SLOTS17 in str(ei.value)


@pytest.mark.parametrize("body", ["auto", "looped"])
def test_seventeen_slots_are_accepted_as_far_as_the_device_under_auto_and_looped(monkeypatch, tmp_path, body):
    monkeypatch.setenv(LC.BODY, body)
    files, inputs = _files(tmp_path)
    device = e.lib.e2vq_device_count() > 0
    for rc in (_posteriors_c([_uniform(64, 8)] * 17, -1.0), _posteriors_c([_uniform(33, 8)] * 17, -1.0), _files_c(files, inputs)):
        if device:
            assert rc == 0, _err()
        else:
            assert rc == 1 and "no HIP device" in _err(), _err()
    # the widest packing the shape check admits passes too: the LDS refusal is out of reach
    rc = _posteriors_c([_uniform(33, 8)] * 124, -1.0)
    assert rc == 0 if device else (rc == 1 and "no HIP device" in _err()), _err()
    # and the other refusals keep their words under the opt-in
    assert _posteriors_c([_uniform(64, 8)] * 65, -1.0) == 1 and "4160 states in all models (at most 4096)" in _err()


# ---- the source and the compiler's metadata --------------------------------------------------------------------------------------
def test_the_restated_lds_formula_is_the_sources():
    src = open(os.path.join(CSRC, "hmm_posterior_looped.hip")).read()
    body = src[src.index("size_t posteriors_looped_lds_bytes("):]
    body = re.sub(r"\s+", " ", body[:body.index("}")])
    assert ("return (size_t)2 * pl.slots * sizeof(double) + (size_t)pl.sumN * sizeof(double) + (a_lds ? (size_t)pl.a_words * 8 : 0);") in body
    assert "const bool a_lds = posteriors_looped_lds_bytes(pl, true) <= SEG_LDS_BYTES;" in src
    assert "const int waves = pl.slots < SEG_MAX_WAVES ? pl.slots : SEG_MAX_WAVES;" in src
    header = open(os.path.join(CSRC, "hmm_device.h")).read()
    assert "constexpr size_t SEG_LDS_BYTES = 160 * 1024;" in header and "constexpr int SEG_MAX_WAVES = 16;" in header
    assert "size_t posteriors_looped_lds_bytes(const SegPlanDev& pl, bool a_lds);" in header and "launch_loop_posteriors_looped(" in header
    assert LC.posteriors_looped_lds_bytes(20, 1280, 20 * 64 * 65, False) == 2 * 20 * 8 + 1280 * 8
    assert LC.posteriors_looped_lds_bytes(17, 561, 17 * 33 * 33, True) == 272 + 4488 + 148104 <= LC.SEG_LDS_BYTES
    r = LC.looped_route([64] * 20)
    assert r == dict(waves=16, a_lds=False, lds=10560, c_copies=16)
    assert LC.looped_route([5] * 3) == dict(waves=1, a_lds=True, lds=16 + 120 + 600, c_copies=1)
    # no class set the shape check admits comes near the limit: the host's LDS refusal cannot be reached
    assert LC.most_mandatory_lds() == 8 * (2 * 129 + 4096) < LC.SEG_LDS_BYTES // 4
    # the host sizes the scratch row by the copies of c_t that the kernel stores: one per wave (body_waves and ForwardTable,
    # written once for every pass with a looped body)
    host = open(os.path.join(CSRC, "hmm_class_loop.cpp")).read()
    assert "int body_waves(bool looped, int slots) { return looped ? std::min(slots, (int)e2hmm::SEG_MAX_WAVES) : slots; }" in host
    assert 'ft.reserve("hmm segment --posteriors", sumN, body_waves(looped, slots), 0, h_offs, S)' in host
    assert "const i64 row = 8 * ((i64)sumN + waves + extra);" in host and "d_c.reserve((size_t)max_frames * waves)" in host


VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_posterior_looped.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_posterior_looped.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


@pytest.mark.parametrize("pattern", [r"k_hmm_loop_posteriors_loopedILb0EE", r"k_hmm_loop_posteriors_loopedILb1EE"])
def test_the_looped_kernels_have_no_scratch_no_spill_and_fit_their_budget(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
    print(pattern, "vgpr", g("vgpr_count"), "sgpr", g("sgpr_count"))


# ---- exports ---------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_exported_and_no_declared_one_is_lost():
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([nm, "-D", "--defined-only", os.path.join(CSRC, "libecoz2vq.so")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    names = set(line.split()[-1] for line in r.stdout.splitlines() if line.strip())
    for part in ("launch_loop_posteriors_looped", "posteriors_looped_lds_bytes", "k_hmm_loop_posteriors_loopedILb0EE",
                 "k_hmm_loop_posteriors_loopedILb1EE", "opt_in_body"):
        assert any(part in n for n in names), part
    # the resident body's launcher and kernels are still there, under their own names
    for part in ("22launch_loop_posteriorsERK", "19posteriors_a_in_ldsERK", "k_hmm_loop_posteriorsILb0EE", "k_hmm_loop_posteriorsILb1EE",
                 "10embed_bodyEPNS_8LoopBodyE"):
        assert any(part in n for n in names), part
    # every function the two public headers declare is exported, the signatures of the posteriors unchanged
    declared = set()
    for h in ("ecoz2_classify.h", "ecoz2_vq.h"):
        declared |= set(re.findall(r"\b(e2vq_\w+|ecoz2_\w+)\s*\(", open(os.path.join(ROOT, "include", h)).read()))
    assert len(declared) > 100 and not sorted(declared - names)
    assert list(inspect.signature(hmm.segment_posteriors).parameters) == ["models", "sym", "offs", "ln_switch", "device", "body"]
    assert inspect.signature(hmm.segment_posteriors).parameters["body"].default is None
    assert inspect.signature(hmm.segment_files).parameters["body"].default is None
    header = open(os.path.join(ROOT, "include", "ecoz2_classify.h")).read()
    assert "ECOZ2_HMM_POSTERIOR_BODY" in header and BAD.replace("fast", "<v>") in header
    assert isinstance(e.lib.e2vq_hmm_segment_posteriors, C._CFuncPtr)
