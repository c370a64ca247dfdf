"""The looped body of `hmm align --posteriors` (ECOZ2_HMM_ALIGN_POSTERIOR_BODY), CPU side: what the opt-in
changes before any HIP call -- the 17-slot refusal goes under `auto` and `looped` and stays, word for word, under `resident` and
with nothing set; the refusals of a bad word, of a transcript whose mandatory LDS does not fit and of `body` without the
posteriors --, the restated LDS sum against the source, the restatement above 16 slots against the laws of the posteriors and
the E-step's restatement, and the new kernel's compiler metadata.  The GPU parity tests are in
test_gpu_hmm_align_posteriors_looped.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_align_cases as cases
from . import hmm_align_posterior_looped_cases as LC
from . import hmm_align_posterior_restatement as PR
from . import hmm_embedded_restatement as ER
from .test_hmm_align_posteriors_cpu import _call, _err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXE = os.path.join(CSRC, "ecoz2")
M = cases.M
WHO = "e2vq_hmm_align_posteriors"
SLOTS = "stream 0: the units take 17 wave-slots of 64 lanes (at most 16: the alignment posteriors have a resident body only)"
uni = lambda N, m=M: (np.full(N, 1.0 / N), np.full((N, N), 1.0 / N), np.full((N, m), 1.0 / m))


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in (LC.BODY, "ECOZ2_HMM_EMBED_A", "ECOZ2_HMM_EMBED_CHUNK_BYTES", "ECOZ2_HMM_ALIGN_BODY"):
        monkeypatch.delenv(k, raising=False)


# ---- before the device -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", ["auto", "looped"])
def test_seventeen_slots_pass_the_plan_under_auto_and_looped(monkeypatch, body):
    """The call ends as a one-slot call ends: the same return value, and without a device the same message."""
    models, units, stream = cases.packing("64x17")
    assert PR.slots_of(models, units) == 17
    one = _call(models, stream, [0, len(stream)], units[:1], [0, 1]), _err()
    assert _call(models, stream, [0, len(stream)], units, [0, 17]) == 1 and _err() == f"{WHO}: {SLOTS}"
    monkeypatch.setenv(LC.BODY, body)
    got = _call(models, stream, [0, len(stream)], units, [0, 17]), _err()
    assert "wave-slots" not in got[1] or got[0] == 0
    assert got[0] == one[0] and (got[0] == 0 or got[1] == one[1]), (got, one)


@pytest.mark.parametrize("body", [None, "", "resident"])
def test_the_old_refusal_comes_word_for_word_with_resident_and_with_nothing_set(monkeypatch, body):
    if body is not None:
        monkeypatch.setenv(LC.BODY, body)
    models, units, stream = cases.packing("64x17")
    assert _call(models, stream, [0, len(stream)], units, [0, 17]) == 1 and _err() == f"{WHO}: {SLOTS}"


def _files(tmp_path):
    for c, N in (("a", 64), ("b", 2)):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *uni(N, 4))
    e.formats.write_seq(str(tmp_path / "x.seq"), "_", 4, np.zeros(40, np.uint16))
    (tmp_path / "wide.csv").write_text("class\n" + "a\n" * 17)
    (tmp_path / "one.csv").write_text("class\na\n")
    return [str(tmp_path / "hmms" / "a.hmm"), str(tmp_path / "hmms" / "b.hmm")], [str(tmp_path / "x.seq")]


def _align(files, seq, lab, **kw):
    try:
        hmm.align_files(files, seq, [str(lab)], posteriors=True, **kw)
        return 0, ""
    except e.Ecoz2Error:
        return 1, _err()


def test_the_file_form_takes_seventeen_labels_through_body_auto(tmp_path):
    files, seq = _files(tmp_path)
    one = _align(files, seq, tmp_path / "one.csv")
    assert _align(files, seq, tmp_path / "wide.csv") == (1, f"{tmp_path / 'wide.csv'}: e2vq_hmm_align_files_posteriors: {SLOTS}")
    got = _align(files, seq, tmp_path / "wide.csv", body="auto")
    assert got == one, (got, one)
    assert LC.BODY not in os.environ  # (the wrapper restores the environment)


def test_a_bad_word_is_refused_byte_for_byte_from_arrays_from_files_and_by_the_cli(monkeypatch, tmp_path):
    models, units, stream = cases.packing("5x13")
    files, seq = _files(tmp_path)
    msg = "ECOZ2_HMM_ALIGN_POSTERIOR_BODY=fast: auto, resident or looped"
    assert _align(files, seq, tmp_path / "one.csv", body="fast") == (1, f"{tmp_path / 'one.csv'}: {msg}")
    with pytest.raises(e.Ecoz2Error):
        hmm.align_posteriors(models, stream, [0, len(stream)], units, [0, len(units)], body="fast")
    assert _err() == msg
    monkeypatch.setenv(LC.BODY, "fast")
    assert _call(models, stream, [0, len(stream)], units, [0, len(units)]) == 1 and _err() == msg
    monkeypatch.delenv(LC.BODY)
    common = [EXE, "hmm", "align", "--models", "hmms", "--labels", "one.csv", "--sequences", "x.seq"]
    r = subprocess.run(common + ["--posteriors", "--body", "fast"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "hmm align --posteriors: --body fast: auto, resident or looped" in r.stderr
    r = subprocess.run(common + ["--body", "auto"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "hmm align: --body <auto|resident|looped> needs --posteriors" in r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert "[--body <auto|resident|looped>]" in (r.stderr + r.stdout).split("ecoz2 hmm align")[1].split("ecoz2 hmm show")[0]
    with pytest.raises(ValueError, match="body needs posteriors=True"):
        hmm.align_files(files, seq, [str(tmp_path / "one.csv")], body="auto")
    assert "ECOZ2_HMM_ALIGN_POSTERIOR_BODY" in hmm._body_env.__doc__


@pytest.mark.parametrize("body", ["auto", "looped"])
def test_a_transcript_whose_mandatory_arrays_do_not_fit_is_refused_before_the_device(monkeypatch, body):
    N, L, slots, sumN = LC.too_large()
    monkeypatch.setenv(LC.BODY, body)
    need = LC.align_post_looped_lds_bytes(L, slots, sumN, 0, False)
    assert need > LC.SEG_LDS_BYTES and need == LC.embed_looped_lds_bytes(L, slots, sumN, 0, False, False) + 24 * L
    assert _call([uni(N)], np.zeros(8, np.uint16), [0, 8], [0] * L, [0, L]) == 1
    assert _err() == (f"{WHO}: stream 0: {L} units of sum N = {sumN} states in {slots} wave-slots do not fit in LDS "
                      f"({need} of {LC.SEG_LDS_BYTES} bytes)")
    # one unit fewer than this pass's bound passes the plan, one more is refused: the per-unit sums are counted (the E-step's
    # own bound lies further out)
    per_slot = 64 // N
    fits = lambda l, f: f(l, -(-l // per_slot), N * l) <= LC.SEG_LDS_BYTES
    post = lambda l, s, n: LC.align_post_looped_lds_bytes(l, s, n, 0, False)
    embed = lambda l, s, n: LC.embed_looped_lds_bytes(l, s, n, 0, False, False)
    fit = max(l for l in range(1, L) if fits(l, post))
    assert fits(fit + 1, embed) and not fits(fit + 1, post)
    rc = _call([uni(N)], np.zeros(8, np.uint16), [0, 8], [0] * fit, [0, fit])
    assert rc == 0 or "do not fit in LDS" not in _err()  # (with a device the call succeeds and leaves the last message alone)
    assert _call([uni(N)], np.zeros(8, np.uint16), [0, 8], [0] * (fit + 1), [0, fit + 1]) == 1 and "do not fit in LDS" in _err()


def test_a_forced_route_of_a_that_does_not_fit_is_refused_on_the_host(monkeypatch):
    models, units, _opt, stream = LC.case("64x6c_17u")
    monkeypatch.setenv(LC.BODY, "auto")
    monkeypatch.setenv("ECOZ2_HMM_EMBED_A", "lds")
    need = LC.align_post_looped_lds_bytes(17, 17, 17 * 64, 6 * 64 * 65, True)
    assert _call(models, stream, [0, len(stream)], units, [0, 17]) == 1
    assert _err() == (f"{WHO}: streams 0 to 0: 17 units of sum N = 1088 states in 17 wave-slots and A in LDS take {need} bytes of LDS "
                      f"(at most {LC.SEG_LDS_BYTES})")


def test_the_embedded_estep_does_not_read_the_variable(monkeypatch):
    models, units, stream = cases.packing("64x17")
    monkeypatch.setenv(LC.BODY, "auto")
    with pytest.raises(Exception, match=r"stream 0: the units take 17 wave-slots of 64 lanes \(at most 16: the embedded E-step has no looped body\)"):
        hmm.embedded_estep(models, stream, [0, len(stream)], units, [0, 17])


# ---- the restatement above 16 slots ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, slots", [("64x17", 17), ("33x20", 20)])
def test_the_restatement_obeys_the_laws_above_sixteen_slots(monkeypatch, name, slots):
    monkeypatch.setattr(PR, "MAX_SLOTS", 64)
    monkeypatch.setattr(ER, "MAX_SLOTS", 64)
    models, units, stream = cases.packing(name)
    assert PR.slots_of(models, units) == slots
    T, L = 120, len(units)
    args = (models, stream[:T], [0, T], units, [0, L], None, -0.5)
    got = PR.posteriors(*args)
    assert got["status"].tolist() == [0]
    assert np.abs(got["occ"][0].sum(axis=1) - 1.0).max() < 1e-12
    assert np.abs(got["present"] - 1.0).max() < 1e-12  # (every unit is mandatory)
    want = ER.estep(*args)
    assert want["status"].tolist() == [0] and got["log_prob"].tobytes() == want["log_prob"].tobytes()


# ---- the source and the compiler's metadata --------------------------------------------------------------------------------------
def test_the_restated_lds_sum_is_the_sources():
    src = open(os.path.join(CSRC, "hmm_align_posterior_looped.hip")).read()
    body = src[src.index("size_t align_post_looped_lds_bytes("):]
    body = re.sub(r"\s+", " ", body[:body.index("}")])
    assert "return embed_looped_lds_bytes(max_L, max_slots, max_sumN, a_words, a_lds, false) + (size_t)3 * max_L * sizeof(double);" in body
    header = open(os.path.join(CSRC, "hmm_device.h")).read()
    assert "constexpr size_t SEG_LDS_BYTES = 160 * 1024;" in header and "constexpr int SEG_MAX_WAVES = 16;" in header
    assert "size_t align_post_looped_lds_bytes(int max_L, int max_slots, int max_sumN, int a_words, bool a_lds);" in header
    assert LC.SEG_LDS_BYTES == 160 * 1024 and LC.SEG_MAX_WAVES == 16 and LC.UNIT_SUM_BYTES == 24
    assert LC.align_post_looped_lds_bytes(20, 20, 660, 5 * 33 * 33, True) == 2 * 20 * 8 * 2 + 2 * 660 * 8 + 3 * 20 * 8 + 5 * 33 * 33 * 8
    # the host hands the plan the bytes a unit adds, and reads the variable through opt_in_body
    host = open(os.path.join(CSRC, "hmm_align_posterior.cpp")).read()
    assert "/*looped_unit_bytes=*/3 * sizeof(double)" in host and "align_post_body(&body)" in host
    assert 'opt_in_body("ECOZ2_HMM_ALIGN_POSTERIOR_BODY", body)' in open(os.path.join(CSRC, "hmm_transcript.cpp")).read()
    # the cases the GPU tests name by their route
    assert LC.looped_route([64] * 6, 17, 17, 17 * 64) is False   # 64x6c_17u: A of 195 KB
    assert LC.looped_route([33] * 5, 20, 20, 660) is True         # 33x20
    assert LC.looped_route([64] * 3, 17, 17, 1088) is True        # 64x17
    assert LC.looped_route([64] * 3, 33, 33, 33 * 64) is True     # 33 slots


VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_align_posterior_looped.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_align_posterior_looped.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


@pytest.mark.parametrize("pattern", [r"k_hmm_align_posteriors_loopedILb0EE", r"k_hmm_align_posteriors_loopedILb1EE"])
def test_the_looped_kernel_has_no_scratch_no_spill_and_fits_its_budget(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
    print(pattern, "vgpr", g("vgpr_count"), "sgpr", g("sgpr_count"))
