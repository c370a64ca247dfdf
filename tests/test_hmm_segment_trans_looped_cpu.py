"""The looped body of `hmm segment --class-transitions` and of its session (DESIGN.md 4.8.8 and 4.8.15,
ECOZ2_HMM_SEGMENT_TRANS_BODY), CPU side: that every wide row's decoded path crosses between a wave's turns in both directions
(from the restatement alone); what the variable changes before any HIP call -- a bad word is refused by the four entry points
that read it, by the Python mirrors and by the CLI; the 17-slot refusal keeps every word with nothing set and under `resident`
and goes under `auto`; the posteriors under the prices never read it --; the CLI's new flag and usage lines; the LDS formula
against the source; the eight new instantiations' compiler metadata; the exports.  The GPU parity tests are in
test_gpu_hmm_segment_trans_looped.py."""
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

from . import hmm_segment_trans_looped_cases as LC
from .test_hmm_segment_trans_cpu import _err, _segment_trans_c, _trans_files, _uniform
from .test_hmm_segment_trans_stream_cpu import _files as _continuous_files
from .test_hmm_segment_trans_stream_cpu import _open_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXE = os.path.join(CSRC, "ecoz2")
SLOTS17 = "the classes take 17 wave-slots of 64 lanes (at most 16: the class-transition decoder has no looped body)"
SLOTS17_POST = "the classes take 17 wave-slots of 64 lanes (at most 16: the posteriors under class-to-class prices have no looped body)"
BAD = "ECOZ2_HMM_SEGMENT_TRANS_BODY=fast: auto, resident or looped"
ENTRY_POINTS = ("e2vq_hmm_segment_trans", "e2vq_hmm_segment_trans_files", "e2vq_hmm_segment_trans_stream_open",
                "e2vq_hmm_segment_trans_continuous_files")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in (LC.BODY, LC.CHUNK, LC.ENV_BLOCK, LC.ENV_PENDING, "ECOZ2_HMM_POSTERIOR_BODY"):
        monkeypatch.delenv(k, raising=False)


# ---- the inputs: a weak row fails here, it does not hide behind a pass on the GPU ------------------------------------------------
@pytest.mark.parametrize("name", list(LC.WIDE))
def test_every_wide_row_is_decoded_across_the_turns_in_both_directions(name):
    Ns, _M, T = LC.WIDE[name]
    ref = LC.wide_reference(name)
    got = LC.crossings(Ns, ref)
    print(name, got)
    assert got["status"] == 0 and len(ref["cls"]) == T
    assert got["slots"] > LC.SEG_MAX_WAVES
    assert got["into_late"] >= 1   # a class in a slot >= 16 is entered ...
    assert got["back_early"] >= 1  # ... and left for a class in a slot < 16


def test_the_wide_sets_are_what_their_comments_say():
    slots = {name: LC.slots_of(Ns) for name, (Ns, _M, _T) in LC.WIDE.items()}
    assert slots == {"64x17": 17, "33x20": 20, "5x204": 17, "mixed_x9": 19, "1x1088": 17, "40_1x24_x18": 18, "64x64": 64}
    per_slot = np.bincount(LC.loop_cases.slot_of_class(LC.WIDE["5x204"][0]))
    assert per_slot.tolist() == [12] * 17
    assert np.bincount(LC.loop_cases.slot_of_class(LC.WIDE["40_1x24_x18"][0])).tolist() == [25] * 18
    assert LC.loop_cases.one_class_slot_next_to_packed(LC.WIDE["mixed_x9"][0])
    assert sum(LC.WIDE["64x64"][0]) == LC.loop_cases.SEG_MAX_SUM_N


# ---- before the device -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def corpus(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    few, many = [], []
    for c in ("A", "B"):
        hmm.save_model(d / f"{c}.hmm", c, *_uniform(3, 16))
        few.append(str(d / f"{c}.hmm"))
    for k in range(17):
        hmm.save_model(d / f"c{k:02d}.hmm", f"c{k:02d}", *_uniform(64, 16))
        many.append(str(d / f"c{k:02d}.hmm"))
    e.formats.write_seq(str(d / "x.seq"), "A", 16, np.arange(40) % 16)
    hmm.write_class_transitions(d / "t2.csv", ["A", "B"], np.zeros((2, 2)))
    hmm.write_class_transitions(d / "t17.csv", [f"c{k:02d}" for k in range(17)], np.zeros((17, 17)))
    return tmp_path, d, few, many


def _four(models, files, transitions, inputs, out):
    """the four entry points that read the variable, in the order of ENTRY_POINTS -> [(rc, message)]"""
    K = len(models)
    res = []
    res.append((_segment_trans_c(models, np.zeros((K, K))), _err()))
    res.append((_trans_files(files, inputs, out, transitions), _err()))
    rc, h = _open_c(models, np.zeros((K, K)))
    res.append((rc, _err()))
    if rc == 0:
        e.lib.e2vq_hmm_segment_stream_free(h)
    res.append((_continuous_files(files, inputs, out, transitions), _err()))
    return res


def test_a_bad_word_is_refused_by_each_entry_point_before_any_hip_call(corpus, monkeypatch):
    tmp_path, d, few, _many = corpus
    monkeypatch.setenv(LC.BODY, "fast")
    out = tmp_path / "out"
    # (this process has no device: a refusal with these words came before the first HIP call, which would have said so)
    for rc, msg in _four([_uniform(3, 8)] * 2, few, d / "t2.csv", [str(d / "x.seq")], out):
        assert rc == 1 and msg == BAD, msg
    assert not out.exists()
    # the earlier checks keep their place: a bad price is seen before the variable
    assert _segment_trans_c([_uniform(3, 8)] * 2, [[0.0, 0.5], [0.0, 0.0]]) == 1 and "lt[0][1] = 0.5" in _err()


@pytest.mark.parametrize("body", [None, "", "resident"])
def test_the_old_refusal_keeps_every_word_with_resident_and_with_nothing_set(corpus, monkeypatch, body):
    tmp_path, d, _few, many = corpus
    if body is not None:
        monkeypatch.setenv(LC.BODY, body)
    out = tmp_path / "out"
    for models in ([_uniform(64, 8)] * 17, [_uniform(33, 8)] * 17):
        res = _four(models, many, d / "t17.csv", [str(d / "x.seq")], out)
        assert [(rc, msg) for rc, msg in res] == [(1, f"{who}: {SLOTS17}") for who in ENTRY_POINTS]
    assert not out.exists()


def test_under_auto_the_widest_sets_pass_every_host_check_and_fail_at_the_device(corpus, monkeypatch):
    tmp_path, d, _few, many = corpus
    monkeypatch.setenv(LC.BODY, "auto")
    device = e.lib.e2vq_device_count() > 0
    out = tmp_path / "out"
    for rc, msg in _four([_uniform(64, 8)] * 17, many, d / "t17.csv", [str(d / "x.seq")], out):
        assert rc == 0 if device else (rc == 1 and "no HIP device" in msg), msg
    for models in ([_uniform(64, 8)] * 64, [_uniform(33, 8)] * 124):  # 4096 states in 64 slots; 124 slots, the most admitted
        K = len(models)
        rc = _segment_trans_c(models, np.zeros((K, K)))
        assert rc == 0 if device else (rc == 1 and "no HIP device" in _err()), _err()
        rc, h = _open_c(models, np.zeros((K, K)))
        assert rc == 0 if device else (rc == 1 and "no HIP device" in _err()), _err()
        if rc == 0:
            e.lib.e2vq_hmm_segment_stream_free(h)
    # the other refusals keep their words under the opt-in
    assert _segment_trans_c([_uniform(64, 8)] * 65, np.zeros((65, 65))) == 1 and "4160 states in all models (at most 4096)" in _err()


def test_the_posteriors_under_the_prices_never_read_the_variable(corpus, monkeypatch):
    tmp_path, d, _few, many = corpus
    for body in ("auto", "looped", "fast"):
        monkeypatch.setenv(LC.BODY, body)
        with pytest.raises(e.Ecoz2Error) as ei:
            hmm.segment_trans_posteriors([_uniform(64, 8)] * 17, np.zeros(8, np.uint16), [0, 8], np.zeros((17, 17)))
        assert SLOTS17_POST in str(ei.value) and _err() == "e2vq_hmm_segment_trans_posteriors: " + SLOTS17_POST
        m, _k1 = hmm._strs(many)
        f, _k2 = hmm._strs([str(d / "x.seq")])
        rc = e.lib.e2vq_hmm_segment_trans_files_posteriors(m, 17, None, f, 1, 4, 45, 15, -5.0, str(d / "t17.csv").encode(),
                                                           str(tmp_path / "out").encode(), None)
        assert rc == 1 and "the classes take 17 wave-slots of 64 lanes (at most 16" in _err() and "no looped body)" in _err()
        assert not (tmp_path / "out").exists()


def test_the_python_mirrors(corpus):
    tmp_path, d, few, many = corpus
    ok = [_uniform(3, 8)] * 2
    with pytest.raises(e.Ecoz2Error):
        hmm.segment_trans(ok, np.zeros(8, np.uint16), [0, 8], np.zeros((2, 2)), body="fast")
    assert _err() == BAD
    with pytest.raises(e.Ecoz2Error):
        hmm.SegmentTransStream(ok, np.zeros((2, 2)), body="fast")
    assert _err() == BAD
    for kw in ({}, dict(grammar_continuous="rec")):
        with pytest.raises(e.Ecoz2Error):
            hmm.segment_files(few, [str(d / "x.seq")], -5.0, csv=tmp_path / "o", class_transitions=d / "t2.csv", grammar_body="fast", **kw)
        assert _err() == BAD and not (tmp_path / "o").exists()
    assert LC.BODY not in os.environ  # (the wrappers restore the environment)
    with pytest.raises(ValueError):
        hmm.segment_files(few, [str(d / "x.seq")], -5.0, grammar_body="auto")  # (no class_transitions)
    with pytest.raises(ValueError):
        hmm.segment_files(few, [str(d / "x.seq")], -5.0, class_transitions=d / "t2.csv", grammar_posteriors=True, grammar_body="auto")
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment_trans([_uniform(64, 8)] * 17, np.zeros(8, np.uint16), [0, 8], np.zeros((17, 17)), body="resident")
    assert SLOTS17 in str(ei.value)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.SegmentTransStream([_uniform(64, 8)] * 17, np.zeros((17, 17)), body="resident")
    assert SLOTS17 in str(ei.value)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------
def _cli(cwd, *args):
    r = subprocess.run([EXE, "hmm", "segment", *args], cwd=cwd, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("args,needle", [
    (["--grammar-body", "auto"], "hmm segment: --grammar-body <auto|resident|looped> needs --class-transitions <file.csv>"),
    (["--grammar-body", "auto", "--posteriors"], "hmm segment: --grammar-body <auto|resident|looped> needs --class-transitions <file.csv>"),
    (["--class-transitions", "in/t2.csv", "--grammar-posteriors", "--grammar-body", "auto"],
     "hmm segment: --grammar-posteriors has the resident body only: not with --grammar-body"),
    (["--class-transitions", "in/t2.csv", "--grammar-body", "fast"],
     "hmm segment --class-transitions: --grammar-body fast: auto, resident or looped"),
    (["--class-transitions", "in/t2.csv", "--grammar-continuous", "rec", "--grammar-body", "fast"],
     "hmm segment --class-transitions: --grammar-body fast: auto, resident or looped"),
    (["--class-transitions", "in/t2.csv", "--grammar-body", ""], "hmm segment --class-transitions: --grammar-body : auto, resident or looped"),
    (["--class-transitions", "in/t2.csv", "--grammar-body"], "--grammar-body needs a value"),
])
def test_cli_refusals_of_the_new_flag(corpus, args, needle):
    tmp_path, _d, _few, _many = corpus
    rc, out, err = _cli(tmp_path, "--models", "in/A.hmm", "in/B.hmm", "--sequences", "in/x.seq", "--switch-penalty", "-5", "-c", "out", *args)
    assert rc == 2 and needle in err, (rc, out, err)
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("args,needle", [
    # --body keeps its meaning and every refusal the earlier tests pin
    (["--body", "auto"], "hmm segment: --body <auto|resident|looped> needs --posteriors"),
    (["--class-transitions", "in/t2.csv", "--grammar-continuous", "rec", "--body", "looped"],
     "hmm segment: --grammar-continuous decodes one stream under the prices of --class-transitions: not with --continuous, "
     "--posteriors, --grammar-posteriors, --frame-posteriors or --body"),
    (["--class-transitions", "in/t2.csv", "--grammar-posteriors", "--body", "auto"],
     "hmm segment: --grammar-posteriors has the resident body and whole recordings only: not with --continuous or --body"),
])
def test_body_keeps_its_refusals(corpus, args, needle):
    tmp_path, _d, _few, _many = corpus
    rc, out, err = _cli(tmp_path, "--models", "in/A.hmm", "in/B.hmm", "--sequences", "in/x.seq", "--switch-penalty", "-5", "-c", "out", *args)
    assert rc == 2 and needle in err, (rc, out, err)


@pytest.mark.parametrize("extra", [[], ["--grammar-body", "resident"], ["--grammar-continuous", "rec"],
                                   ["--grammar-continuous", "rec", "--grammar-body", "resident"]])
def test_cli_seventeen_slots_without_the_opt_in_exit_1_with_the_old_words(corpus, extra):
    tmp_path, _d, _few, _many = corpus
    rc, out, err = _cli(tmp_path, "--models", *[f"in/c{k:02d}.hmm" for k in range(17)], "--sequences", "in/x.seq", "--switch-penalty", "-5",
                        "-c", "out", "--class-transitions", "in/t17.csv", *extra)
    assert rc == 1 and SLOTS17 in out, (rc, out, err)
    assert not (tmp_path / "out").exists()


def test_usage_gains_lines_and_keeps_every_pinned_one(tmp_path):
    rc, _out, err = _cli(tmp_path)
    assert rc == 2
    old = ("  ecoz2 hmm segment -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15]\n"
           "                  --switch-penalty <x <= 0 | -inf> [-c <csv dir|file.csv>]\n"
           "                  [--posteriors [--frame-posteriors <dir>]]\n"
           "                  [--body <auto|resident|looped>]\n"
           "                  [--class-transitions <file.csv>]\n"
           "                  [--grammar-posteriors [--frame-posteriors <dir>]]\n"
           "                  [--continuous <name>]\n")
    assert old + "                  [--grammar-body <auto|resident|looped>]\n" in err
    stream = ("  ecoz2 hmm segment -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15]\n"
              "                  --switch-penalty <x <= 0 | -inf> --class-transitions <file.csv> --grammar-continuous <name>\n"
              "                  [-c <csv dir|file.csv>]\n"
              "                  [--grammar-body <auto|resident|looped>]\n")
    assert stream in err and err.index(old) < err.index(stream) < err.index("  ecoz2 hmm transitions -m|--models")
    assert "                  (--grammar-body, with --class-transitions: the kernel body of the decoder under the prices -- resident\n" in err
    for line in ("                  (--continuous <name>: the inputs are consecutive pieces of one recording, decoded as one stream)\n",
                 "                  (--grammar-continuous <name>: the inputs are consecutive pieces of one recording, decoded as one stream\n",
                 "                  under the prices of --class-transitions)\n",
                 "                  (--body, with --posteriors: the kernel body of the posteriors -- resident takes at most 16 wave-slots\n",
                 "                  (--class-transitions adds the file's price of every class-to-class succession to the penalty)\n",
                 "                  --posteriors adds each segment's mean and least class posterior, and the per-frame table)\n"):
        assert line in err, line


# ---- the source and the compiler's metadata --------------------------------------------------------------------------------------
def test_the_restated_lds_formula_is_the_sources():
    src = open(os.path.join(CSRC, "hmm_segment_trans_looped.hip")).read()
    body = src[src.index("size_t segment_trans_looped_lds_bytes("):]
    body = re.sub(r"\s+", " ", body[:body.index("}")])
    assert ("return (size_t)SEG_MAX_WAVES * sizeof(Pair) + (size_t)2 * pl.K * 8 + (size_t)pl.sumN * (8 + 8 + 4) + "
            "(a_lds ? (size_t)pl.a_words * 8 : 0) + (lt_lds ? (size_t)pl.K * pl.K * 8 : 0);") in body
    layout = re.sub(r"\s+", " ", src[src.index("void segment_trans_looped_layout("):])
    assert "*a_lds = segment_trans_looped_lds_bytes(pl, true, false) <= SEG_LDS_BYTES;" in layout  # A first,
    assert "*lt_lds = segment_trans_looped_lds_bytes(pl, *a_lds, true) <= SEG_LDS_BYTES;" in layout  # then ltT
    assert src.count("const size_t lds = segment_trans_looped_lds_bytes(pl, a_lds, lt_lds);") == 2  # both launchers
    assert src.count("const int waves = pl.slots < SEG_MAX_WAVES ? pl.slots : SEG_MAX_WAVES;") == 2
    header = open(os.path.join(CSRC, "hmm_device.h")).read()
    assert "constexpr size_t SEG_LDS_BYTES = 160 * 1024;" in header and "constexpr int SEG_MAX_WAVES = 16;" in header
    assert "size_t segment_trans_looped_lds_bytes(const SegPlanDev& pl, bool a_lds, bool lt_lds);" in header
    host = open(os.path.join(CSRC, "hmm_class_loop.cpp")).read()
    assert "e2hmm::segment_trans_looped_lds_bytes(shape, false, false)" in host  # the host's check is the launcher's formula
    assert LC.PAIR_BYTES == 16
    # every row: which of A / lt are staged, and the bytes of the launch
    T, F = True, False
    want = {"64x17": (F, T, 24600), "33x20": (F, T, 16976), "5x204": (T, F, 64720), "mixed_x9": (F, T, 37696),
            "1x1088": (T, F, 48128), "40_1x24_x18": (F, F, 30496), "64x64": (F, T, 115968)}
    for name, (Ns, _M, _T) in LC.WIDE.items():
        r = LC.looped_route(Ns)
        assert (r["a_lds"], r["lt_lds"], r["lds"]) == want[name] and r["waves"] == 16, (name, r)
    assert LC.segment_trans_looped_lds_bytes(17, 1088, 17 * 4096, False, True) == 256 + 16 * 17 + 20 * 1088 + 8 * 17 * 17
    # forced below the cap, the four placements: (A, lt) = TT, FT, TF, FF
    below = {"5x12": [5] * 12, "64x16": [64] * 16, "1x1024": [1] * 1024, "40_1x24_x14": ([40] + [1] * 24) * 14}
    got = {k: (LC.looped_route(Ns)["a_lds"], LC.looped_route(Ns)["lt_lds"]) for k, Ns in below.items()}
    assert got == {"5x12": (T, T), "64x16": (F, T), "1x1024": (T, F), "40_1x24_x14": (F, F)}
    assert LC.looped_route([5] * 12)["waves"] == 1 and LC.looped_route([64] * 16)["waves"] == 16
    # no class set the shape check admits reaches the limit: the host's LDS refusal cannot be reached
    assert LC.most_mandatory_lds() == 256 + 16 * 4096 + 20 * 4096 == 147712 < LC.SEG_LDS_BYTES == 163840


VGPR_BUDGET = 128  # 16 waves of one workgroup on a CU: four a SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_segment_trans_looped.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_segment_trans_looped.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


@pytest.mark.parametrize("pattern", [f"{k}ILb{a}ELb{l}EE" for k in ("k_hmm_segment_trans_looped", "k_hmm_segment_trans_stream_looped")
                                     for a in (0, 1) for l in (0, 1)])
def test_the_looped_kernels_have_no_scratch_no_spill_and_fit_their_budget(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")
    print(pattern, "vgpr", g("vgpr_count"), "sgpr", g("sgpr_count"))


# ---- exports ---------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_exported_and_the_signatures_are_what_the_mirrors_say():
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([nm, "-D", "--defined-only", os.path.join(CSRC, "libecoz2vq.so")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    names = set(line.split()[-1] for line in r.stdout.splitlines() if line.strip())
    for part in ("launch_segment_trans_looped", "launch_segment_trans_stream_looped", "segment_trans_looped_lds_bytes",
                 "segment_trans_looped_layout", "segment_trans_body", "trans_check_slots",
                 *[f"{k}ILb{a}ELb{l}EE" for k in ("k_hmm_segment_trans_looped", "k_hmm_segment_trans_stream_looped") for a in (0, 1) for l in (0, 1)]):
        assert any(part in n for n in names), part
    # the resident bodies are still there, under their own names
    for part in ("20launch_segment_transERK", "27launch_segment_trans_streamERK", "k_hmm_segment_transILb0ELb0EE", "k_hmm_segment_trans_streamILb1ELb1EE",
                 "k_hmm_segment_trans_coalesce", "k_hmm_segment_trans_stream_backtrack", "k_hmm_segment_trans_backtrack"):
        assert any(part in n for n in names), part
    declared = set()
    for h in ("ecoz2_classify.h", "ecoz2_vq.h"):
        declared |= set(re.findall(r"\b(e2vq_\w+|ecoz2_\w+)\s*\(", open(os.path.join(ROOT, "include", h)).read()))
    assert len(declared) > 100 and not sorted(declared - names)
    assert list(inspect.signature(hmm.segment_trans).parameters) == ["models", "sym", "offs", "ln_trans", "device", "body"]
    assert list(inspect.signature(hmm.SegmentTransStream.__init__).parameters) == ["self", "models", "ln_trans", "device", "body"]
    for fn in (hmm.segment_trans, hmm.SegmentTransStream.__init__):
        assert inspect.signature(fn).parameters["body"].default is None
    assert inspect.signature(hmm.segment_files).parameters["grammar_body"].default is None
    assert list(inspect.signature(hmm.segment_trans_posteriors).parameters) == ["models", "sym", "offs", "ln_trans", "device"]
    header = open(os.path.join(ROOT, "include", "ecoz2_classify.h")).read()
    assert LC.BODY in header and BAD.replace("fast", "<v>") in header
    for name in ENTRY_POINTS:
        assert isinstance(getattr(e.lib, name), C._CFuncPtr)
