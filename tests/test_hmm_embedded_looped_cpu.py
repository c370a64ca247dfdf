"""The looped body of the embedded E-step (ECOZ2_HMM_EMBED_BODY), CPU side: what the opt-in changes before any
HIP call -- the 17-slot refusal goes under `auto` and `looped` and stays, word for word, under `resident` and with nothing set;
the refusals of a bad word and of a transcript whose mandatory LDS does not fit; `hmm align --posteriors` does not read the
variable --, the restatement at 17 and 33 slots against the contract in plain loops, what the GPU tests rely on in the random
batch, the LDS formula against the source, and the new kernel's compiler metadata.  The GPU parity tests are in
test_gpu_hmm_embedded_looped.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_embedded_cases as cases
from . import hmm_embedded_looped_cases as LC
from . import hmm_embedded_restatement as R
from .test_hmm_embedded_cpu import _call, _err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXE = os.path.join(CSRC, "ecoz2")
M = cases.M
SLOTS = "stream 0: the units take 17 wave-slots of 64 lanes (at most 16: the embedded E-step has no looped body)"
uni = lambda N, m=M: (np.full(N, 1.0 / N), np.full((N, N), 1.0 / N), np.full((N, m), 1.0 / m))


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in (LC.BODY, "ECOZ2_HMM_EMBED_A", "ECOZ2_HMM_EMBED_AN", "ECOZ2_HMM_EMBED_CHUNK_BYTES"):
        monkeypatch.delenv(k, raising=False)


# ---- before the device -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", ["auto", "looped"])
@pytest.mark.parametrize("train", [False, True])
def test_seventeen_slots_pass_the_plan_under_auto_and_looped(monkeypatch, body, train):
    """The call ends as a one-slot call ends: the same return value, and without a device the same message."""
    models, units, stream = cases.packing("64x17")
    assert R.slots_of(models, units) == 17
    one = _call(models, stream, [0, len(stream)], units[:1], [0, 1], train=train), _err()
    assert _call(models, stream, [0, len(stream)], units, [0, 17], train=train) == 1 and _err().endswith(SLOTS)
    monkeypatch.setenv(LC.BODY, body)
    got = _call(models, stream, [0, len(stream)], units, [0, 17], train=train), _err()
    assert "wave-slots" not in got[1] or got[0] == 0
    assert got[0] == one[0] and (got[0] == 0 or got[1] == one[1]), (got, one)


def _files(tmp_path):
    for c, N in (("a", 64), ("b", 2)):
        hmm.save_model(tmp_path / f"{c}.hmm", c, *uni(N, 4))
    e.formats.write_seq(str(tmp_path / "x.seq"), "_", 4, np.zeros(40, np.uint16))
    (tmp_path / "wide.csv").write_text("class\n" + "a\n" * 17)
    (tmp_path / "one.csv").write_text("class\na\n")
    return [str(tmp_path / "a.hmm"), str(tmp_path / "b.hmm")], [str(tmp_path / "x.seq")]


def _learn(files, seq, lab, out, **kw):
    try:
        hmm.learn_embedded_files(files, seq, [str(lab)], out, max_iterations=1, **kw)
        return 0, ""
    except e.Ecoz2Error:
        return 1, _err()


def test_the_file_form_takes_seventeen_labels_through_body_auto(tmp_path):
    files, seq = _files(tmp_path)
    one = _learn(files, seq, tmp_path / "one.csv", tmp_path / "o1")
    assert _learn(files, seq, tmp_path / "wide.csv", tmp_path / "o2") == (1, f"{tmp_path / 'wide.csv'}: e2vq_hmm_learn_embedded_files: {SLOTS}")
    got = _learn(files, seq, tmp_path / "wide.csv", tmp_path / "o3", body="auto")
    assert got == one, (got, one)
    assert LC.BODY not in os.environ  # (the wrapper restores the environment)


def test_a_bad_word_is_refused_byte_for_byte_from_arrays_from_files_and_by_the_cli(monkeypatch, tmp_path):
    models, units, stream = cases.packing("5x13")
    files, seq = _files(tmp_path)
    msg = "ECOZ2_HMM_EMBED_BODY=fast: auto, resident or looped"
    assert _learn(files, seq, tmp_path / "one.csv", tmp_path / "o", body="fast") == (1, f"{tmp_path / 'one.csv'}: {msg}")
    with pytest.raises(e.Ecoz2Error):
        hmm.embedded_estep(models, stream, [0, len(stream)], units, [0, len(units)], body="fast")
    assert _err() == msg
    monkeypatch.setenv(LC.BODY, "fast")
    for train in (False, True):
        assert _call(models, stream, [0, len(stream)], units, [0, len(units)], train=train) == 1 and _err() == msg
    assert not (tmp_path / "o").exists()
    monkeypatch.delenv(LC.BODY)
    r = subprocess.run([EXE, "hmm", "learn", "--embedded", "--models", "hmms", "--labels", "x.csv", "-o", "o", "--sequences", "x.seq", "--body", "fast"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--body fast: auto, resident or looped" in r.stderr and "ecoz2 hmm learn --embedded" in r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert "[--body <auto|resident|looped>]" in r.stderr + r.stdout


@pytest.mark.parametrize("body", [None, "", "resident"])
def test_the_old_refusal_comes_word_for_word_with_resident_and_with_nothing_set(monkeypatch, body):
    if body is not None:
        monkeypatch.setenv(LC.BODY, body)
    models, units, stream = cases.packing("64x17")
    for train, who in ((False, "e2vq_hmm_embedded_estep"), (True, "e2vq_hmm_train_embedded")):
        assert _call(models, stream, [0, len(stream)], units, [0, 17], train=train) == 1
        assert _err() == f"{who}: {SLOTS}"


@pytest.mark.parametrize("body", ["auto", "looped"])
def test_a_transcript_whose_per_state_arrays_do_not_fit_is_refused_before_the_device(monkeypatch, body):
    N, L, slots, sumN = LC.too_large()
    monkeypatch.setenv(LC.BODY, body)
    need = LC.embed_looped_lds_bytes(L, slots, sumN, 0, False, False)
    assert _call([uni(N)], np.zeros(8, np.uint16), [0, 8], [0] * L, [0, L]) == 1
    assert _err() == (f"e2vq_hmm_embedded_estep: stream 0: {L} units of sum N = {sumN} states in {slots} wave-slots do not fit in LDS "
                      f"({need} of {LC.SEG_LDS_BYTES} bytes)")
    # one unit fewer than the formula's bound passes the plan: the refusal is the formula's, not a round number's
    per_slot = 64 // N
    fit = max(l for l in range(1, L) if LC.embed_looped_lds_bytes(l, -(-l // per_slot), N * l, 0, False, False) <= LC.SEG_LDS_BYTES)
    assert cases.slots_of([N] * fit) == -(-fit // per_slot)
    rc = _call([uni(N)], np.zeros(8, np.uint16), [0, 8], [0] * fit, [0, fit])
    assert rc == 0 or "do not fit in LDS" not in _err()  # (with a device the call succeeds and leaves the last message alone)
    assert _call([uni(N)], np.zeros(8, np.uint16), [0, 8], [0] * (fit + 1), [0, fit + 1]) == 1 and "do not fit in LDS" in _err()


def test_the_alignment_posteriors_do_not_read_the_variable(monkeypatch):
    models, units, stream = cases.packing("64x17")
    monkeypatch.setenv(LC.BODY, "auto")
    with pytest.raises(Exception, match=r"stream 0: the units take 17 wave-slots of 64 lanes \(at most 16: the alignment posteriors have a "
                                        r"resident body only\)"):
        hmm.align_posteriors(models, stream, [0, len(stream)], units, [0, 17])
    monkeypatch.setenv(LC.BODY, "fast")  # (not even a bad word is seen)
    with pytest.raises(Exception, match="resident body only"):
        hmm.align_posteriors(models, stream, [0, len(stream)], units, [0, 17])


# ---- the restatement above 16 slots ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L, optional, T", [(17, False, 18), (33, True, 17)], ids=["17 slots", "33 slots"])
def test_the_restatement_is_the_transcription_above_sixteen_slots(monkeypatch, L, optional, T):
    """units of 33 states take a slot each; at 33 slots every other unit is optional, so that 17 frames have a path"""
    monkeypatch.setattr(R, "MAX_SLOTS", 64)
    models = cases.small_models(seed=L, Ns=(33, 33), zeros=0.2)
    units = np.array([l % 2 for l in range(L)], np.int32)
    opt = np.array([l % 2 == 0 for l in range(L)], np.uint8) if optional else None
    assert R.slots_of(models, units) == L
    seq = np.random.default_rng(L).integers(0, M, T)
    args = (models, seq, [0, T], units, [0, L], opt, -0.5)
    a, b = R.estep(*args), R.estep(*args, one=R.transcribe)
    assert a["status"].tolist() == b["status"].tolist() == [0] and a["log_prob"].tobytes() == b["log_prob"].tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(a["acc"], b["acc"]))


def test_the_random_batch_has_what_the_gpu_test_relies_on(monkeypatch):
    monkeypatch.setattr(R, "MAX_SLOTS", 64)
    models, streams, transcripts, optionals = cases.random_batch(LC.RANDOM_SEED, LC.RANDOM_MAX_L)
    slots = [R.slots_of(models, u) for u in transcripts]
    assert len(streams) == 40 and sum(s > 16 for s in slots) == 5 and max(slots) <= 20
    want = R.estep(models, *cases.pack(streams, transcripts, optionals), -1.0)
    assert want["status"].tolist() == [0] * 40


# ---- the source and the compiler's metadata --------------------------------------------------------------------------------------
def test_the_restated_lds_formula_is_the_sources():
    src = open(os.path.join(CSRC, "hmm_embed_looped.hip")).read()
    body = src[src.index("size_t embed_looped_lds_bytes("):]
    body = re.sub(r"\s+", " ", body[:body.index("}")])
    assert ("return (size_t)2 * max_slots * sizeof(double) + (size_t)2 * max_L * 8 + (size_t)2 * max_sumN * 8 + "
            "(a_lds ? (size_t)a_words * 8 : 0) + (an_lds ? (size_t)a_words * 16 : 0);") in body
    header = open(os.path.join(CSRC, "hmm_device.h")).read()
    assert "constexpr size_t SEG_LDS_BYTES = 160 * 1024;" in header and "constexpr int SEG_MAX_WAVES = 16;" in header
    assert LC.embed_looped_lds_bytes(20, 20, 660, 5 * 33 * 33, True, True) == 2 * 20 * 8 * 2 + 2 * 660 * 8 + 5 * 33 * 33 * 24
    # the cases the GPU tests name by their route
    Ns = [64] * 6
    assert LC.looped_route(Ns, 17, 17, 17 * 64) == (False, False)   # 64x6c_17u: A of 192 KB
    assert LC.looped_route([33] * 5, 20, 20, 660) == (True, True)    # 33x20
    assert LC.looped_route([64] * 3, 17, 17, 1088) == (True, False)  # 64x17: A in LDS, no room for the AN table


VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_embed_looped.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_embed_looped.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


@pytest.mark.parametrize("pattern", [r"k_hmm_embed_fb_loopedILb0EE", r"k_hmm_embed_fb_loopedILb1EE"])
def test_the_looped_kernel_has_no_scratch_no_spill_and_fits_its_budget(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
    print(pattern, "vgpr", g("vgpr_count"), "sgpr", g("sgpr_count"))
