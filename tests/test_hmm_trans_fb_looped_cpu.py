"""The looped bodies of the forward-backward passes under class-to-class prices (DESIGN.md 4.8.13 and 4.8.14,
ECOZ2_HMM_TRANS_FB_BODY), CPU side: that every wide row's references light classes and cells on both sides of the sixteenth
slot (from the restatements alone); the LDS formulas against the source of the new launchers; what the variable changes before
any HIP call at the five entry points that read it -- the 17-slot refusals keep every word with nothing set and under
`resident`, a bad word is refused with opt_in_body's words, `auto` and `looped` reach the device --; that the two other body
variables are never read by these calls; the Python keywords and the restored environment; the CLI's two flags; the exports.
The GPU parity tests are in test_gpu_hmm_trans_fb_looped.py."""
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

from . import hmm_trans_fb_looped_cases as FC
from .test_hmm_segment_trans_cpu import _err, _uniform
from .test_hmm_trans_posteriors_cpu import _call_c as _posteriors_c
from .test_hmm_transitions_em_cpu import _call_c as _estep_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
EXE = os.path.join(CSRC, "ecoz2")
SLOTS17 = "the classes take 17 wave-slots of 64 lanes (at most 16: "
SLOTS17_POST = SLOTS17 + "the posteriors under class-to-class prices have no looped body)"
SLOTS17_ESTEP = SLOTS17 + "the E-step of the class transitions has no looped body)"
SLOTS17_DECODE = SLOTS17 + "the class-transition decoder has no looped body)"
BAD = "ECOZ2_HMM_TRANS_FB_BODY=fast: auto, resident or looped"
ENTRY_POINTS = ("e2vq_hmm_segment_trans_posteriors", "e2vq_hmm_segment_trans_files_posteriors", "e2vq_hmm_transitions_estep",
                "e2vq_hmm_train_transitions", "e2vq_hmm_learn_transitions_files")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in (FC.BODY, FC.CHUNK, FC.ROUTE_C, *FC.OTHER_BODIES):
        monkeypatch.delenv(k, raising=False)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- the inputs: a weak row fails here, it does not hide behind a pass on the GPU ------------------------------------------------
@pytest.mark.parametrize("name", list(FC.WIDE))
def test_every_wide_row_lights_both_sides_of_the_sixteenth_slot(name):
    Ns, _M = FC.WIDE[name]
    post, est = FC.wide_posteriors(name), FC.wide_estep(name)
    got = FC.coverage(name)
    print(name, got)
    assert FC.slots_of(Ns) == FC.SLOTS[name] > FC.SEG_MAX_WAVES
    assert post["status"].tolist() == est["status"].tolist() == [0] * len(FC.LENGTHS)
    assert np.array_equal(_bits(post["log_prob"]), _bits(est["log_prob"]))  # stream by stream
    assert got["post_late"] >= 0.1 and got["post_early"] >= 0.1
    assert got["into_late"] >= 1 and got["back_early"] >= 1
    K = len(Ns)
    assert est["acc"][2 * K * K:].tolist() == [len(FC.LENGTHS), 0]
    assert FC.TP.MAX_SLOTS == FC.TE.MAX_SLOTS == 16  # (the cap is lifted for the calls only)


def test_the_rows_are_what_their_comments_say():
    Ns = {name: row[0] for name, row in FC.WIDE.items()}
    assert np.bincount(FC.loop_cases.slot_of_class(Ns["5x204"])).tolist() == [12] * 17
    assert np.bincount(FC.loop_cases.slot_of_class(Ns["8x136"])).tolist() == [8] * 17
    assert FC.loop_cases.one_class_slot_next_to_packed(Ns["mixed_x9"])
    assert sum(Ns["64x64"]) == FC.loop_cases.SEG_MAX_SUM_N and sum(Ns["33x124"]) + 33 > FC.loop_cases.SEG_MAX_SUM_N
    T, F = True, False
    route = {name: FC.looped_route(n) for name, n in Ns.items()}
    assert all(r["waves"] == 16 for r in route.values())
    # (A, w, bytes) of the posteriors | (C, A, w, bytes) of the E-step
    assert {k: (r["post"], r["estep"]) for k, r in route.items()} == {
        "64x17": ((F, T, 13872), (T, F, T, 27200)), "33x17": ((T, T, 157760), (T, T, F, 162248)),
        "33x20": ((F, T, 12320), (T, F, T, 24000)), "5x204": ((T, F, 52496), (F, T, F, 60656)),
        "8x136": ((T, F, 89488), (F, T, F, 98192)), "mixed_x9": ((F, T, 41632), (T, F, T, 82240)),
        "33x33": ((F, T, 27192), (T, F, T, 53328)), "64x64": ((F, T, 100352), (T, F, F, 133120)),
        "33x124": ((F, F, 36704), (F, F, F, 69440))}
    # between them the rows reach A, w and C in LDS and in global memory, in either pass
    for i in (0, 1):
        assert {r["post"][i] for r in route.values()} == {T, F}
    for i in (0, 1, 2):
        assert {r["estep"][i] for r in route.values()} == {T, F}
    assert FC.looped_route(Ns["64x17"], c=False)["estep"] == (F, F, T, 22576)  # ECOZ2_HMM_TRANS_EM_C=global
    # no class set the shape check admits reaches the limit: the hosts' LDS refusals cannot be reached
    assert FC.most_mandatory_lds() == (100368, 133136) and max(FC.most_mandatory_lds()) < FC.SEG_LDS_BYTES == 163840
    assert FC.posteriors_trans_looped_lds_bytes(64, 4096, 4096, 0, F, F) == 99328
    assert FC.trans_estep_looped_lds_bytes(64, 4096, 4096, 0, F, F, F) == 132096


@pytest.mark.parametrize("name", FC.EVENT_ROWS)
def test_the_event_batches_fail_where_they_should(name):
    models, sym, offs, lt, kinds = FC.event_case(name)
    Ns, M = FC.WIDE[name]
    post, est = FC.event_posteriors(name), FC.event_estep(name)
    want = [{"clean": 0, "M": 2, "dead": 1}[k] for k in kinds]
    assert post["status"].tolist() == est["status"].tolist() == want
    assert kinds.count("M") == kinds.count("dead") == len(FC.EVENT_AT) and kinds[0] == kinds[-1] == "clean"
    K = len(Ns)
    assert est["acc"][2 * K * K:].tolist() == [3, 10]
    late = FC.loop_cases.slot_of_class(Ns) >= FC.SEG_MAX_WAVES
    dead = [s for s, k in enumerate(kinds) if k == "dead"]
    for s, p in zip(dead, FC.EVENT_AT):
        a = int(offs[s])
        assert sym[a + p] == M - 1 and (post["post"][a:a + FC.EVENT_T] == 0.0).all()
        if p == 0:
            continue
        # the frames before the dead one are alive, and all their mass sits in the slots >= 16
        before = FC.posteriors(models, sym[a:a + p], [0, p], lt)
        assert before["status"].tolist() == [0]
        assert (before["post"][:, ~late] == 0.0).all() and before["post"][:, late].sum() > 0.99 * p


def test_the_planted_training_never_falls():
    ln_p, hist = FC.train_reference()
    assert len(hist) == FC.TRAIN_ITERATIONS and hist[0] <= hist[1] <= hist[2] and hist[2] > hist[0] + 1.0
    assert ln_p.shape == (17, 17)


# ---- the LDS formulas against the source -----------------------------------------------------------------------------------------
def _flat(text):
    return re.sub(r"\s+", " ", text)


def test_the_restated_lds_formulas_are_the_sources():
    post = open(os.path.join(CSRC, "hmm_posterior_trans_looped.hip")).read()
    body = _flat(post[post.index("size_t posteriors_trans_looped_lds_bytes("):])
    assert ("return ((size_t)2 * pl.slots + (size_t)2 * pl.K + (size_t)pl.sumN + (a_lds ? (size_t)pl.a_words : 0) + "
            "(w_lds ? (size_t)2 * pl.K * pl.K : 0)) * sizeof(double);") in body[:body.index("}")]
    layout = _flat(post[post.index("void posteriors_trans_looped_layout("):])
    assert "*a_lds = posteriors_trans_looped_lds_bytes(pl, true, false) <= SEG_LDS_BYTES;" in layout  # A first,
    assert "*w_lds = posteriors_trans_looped_lds_bytes(pl, *a_lds, true) <= SEG_LDS_BYTES;" in layout  # then w with wT
    launcher = _flat(post[post.index("int launch_loop_posteriors_trans_looped("):])
    assert "posteriors_trans_looped_lds_bytes(pl, false, false) > SEG_LDS_BYTES) return 1;" in launcher
    assert "const size_t lds = posteriors_trans_looped_lds_bytes(pl, a_lds, w_lds);" in launcher
    est = open(os.path.join(CSRC, "hmm_trans_estep_looped.hip")).read()
    body = _flat(est[est.index("size_t trans_estep_looped_lds_bytes("):])
    assert ("return ((size_t)2 * pl.slots + (size_t)2 * pl.K + (size_t)2 * pl.sumN + (c_lds ? (size_t)2 * pl.K * pl.K : 0) + "
            "(a_lds ? (size_t)pl.a_words : 0) + (w_lds ? (size_t)2 * pl.K * pl.K : 0)) * sizeof(double);") in body[:body.index("}")]
    layout = _flat(est[est.index("void trans_estep_looped_layout("):])
    assert "if (!c_forced) *c_lds = trans_estep_looped_lds_bytes(pl, true, false, false) <= SEG_LDS_BYTES;" in layout  # C first,
    assert "*a_lds = trans_estep_looped_lds_bytes(pl, *c_lds, true, false) <= SEG_LDS_BYTES;" in layout                # then A,
    assert "*w_lds = trans_estep_looped_lds_bytes(pl, *c_lds, *a_lds, true) <= SEG_LDS_BYTES;" in layout               # then w
    launcher = _flat(est[est.index("int launch_trans_estep_looped("):])
    assert "const size_t lds = trans_estep_looped_lds_bytes(pl, c_lds, a_lds, w_lds); if (lds > SEG_LDS_BYTES) return 1;" in launcher
    for src in (post, est):  # min(slots, 16) waves, and the kernels carve LDS in the formulas' order
        assert src.count("const int waves = pl.slots < SEG_MAX_WAVES ? pl.slots : SEG_MAX_WAVES;") == 1
        assert "block((unsigned)(64 * waves))" in src
        assert "tb.Xb = tb.parts + 2 * (size_t)slots;" in src and "tb.sv = tb.Xb + 2 * (size_t)K;" in src
    assert "double* As = tb.sv + sumN;" in post
    assert "double* sS = tb.sv + sumN;" in est and "i64* Cs = (i64*)(sS + sumN);" in est
    header = open(os.path.join(CSRC, "hmm_device.h")).read()
    assert "constexpr size_t SEG_LDS_BYTES = 160 * 1024;" in header and "constexpr int SEG_MAX_WAVES = 16;" in header
    assert "size_t posteriors_trans_looped_lds_bytes(const SegPlanDev& pl, bool a_lds, bool w_lds);" in header
    assert "size_t trans_estep_looped_lds_bytes(const SegPlanDev& pl, bool c_lds, bool a_lds, bool w_lds);" in header
    # the hosts' checks are the launchers' formulas, and c_t is stored once per wave
    host = open(os.path.join(CSRC, "hmm_class_loop.cpp")).read()
    assert "e2hmm::posteriors_trans_looped_lds_bytes(shape, false, false)" in host
    train = open(os.path.join(CSRC, "hmm_trans_train.cpp")).read()
    assert "lds_bytes = tp.looped ? e2hmm::trans_estep_looped_lds_bytes : e2hmm::trans_estep_lds_bytes;" in train
    assert "e2hmm::trans_estep_looped_lds_bytes(shape, false, false, false)" in train  # (what check_body_slots holds against the limit)
    assert "if (looped_lds <= e2hmm::SEG_LDS_BYTES) return 0;" in host
    # (body_waves and ForwardTable: written once in hmm_class_loop.cpp for every pass with a looped body)
    assert "int body_waves(bool looped, int slots) { return looped ? std::min(slots, (int)e2hmm::SEG_MAX_WAVES) : slots; }" in host
    assert "const i64 row = 8 * ((i64)sumN + waves + extra);" in host and "d_c.reserve((size_t)max_frames * waves)" in host
    assert 'ft.reserve("hmm segment --grammar-posteriors", sumN, body_waves(looped, slots), 0, h_offs, S)' in host
    assert "tp.waves = body_waves(tp.looped, tp.pk.slots);" in train and "ft.reserve(who, tp.pk.sumN, tp.waves, 0, h_offs, S)" in train
    # the frame is written once, and the units are compiled like their siblings
    for src in (post, est):
        assert '#include "hmm_trans_fb_looped_step.h"' in src and "fb_forward_frame(" in src and "fb_post_R(" in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "hmm_posterior_trans_looped.o" in mk and "hmm_trans_estep_looped.o" in mk and "hmm_trans_fb_looped_step.h" in mk
    assert "-ffp-contract=off" in mk


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


def _five(models, files, transitions, inputs, out):
    """the five entry points that read the variable, in the order of ENTRY_POINTS -> [(rc, message)]"""
    K = len(models)
    z = np.full((K, K), -1.0)
    m, _k1 = hmm._strs(files)
    f, _k2 = hmm._strs(inputs)
    res = [(_posteriors_c(models, z), _err())]
    res.append((e.lib.e2vq_hmm_segment_trans_files_posteriors(m, len(files), None, f, len(inputs), 4, 45, 15, -5.0,
                                                              str(transitions).encode(), str(out / "seg").encode(), None), _err()))
    res.append((_estep_c(models, z), _err()))
    res.append((_estep_c(models, z, train=True), _err()))
    res.append((e.lib.e2vq_hmm_learn_transitions_files(m, len(files), None, f, len(inputs), 4, 45, 15, -5.0, None, 1.0, 0.3, 1,
                                                       str(out / "t.csv").encode()), _err()))
    return res


def _old_words(who):
    # (the file entry point of the posteriors checks its decoder first: the same sentence with the decoder's clause)
    clause = {"e2vq_hmm_segment_trans_posteriors": SLOTS17_POST, "e2vq_hmm_segment_trans_files_posteriors": SLOTS17_DECODE}
    return f"{who}: {clause.get(who, SLOTS17_ESTEP)}"


@pytest.mark.parametrize("body", [None, "", "resident"])
def test_the_old_refusals_keep_every_word_with_resident_and_with_nothing_set(corpus, monkeypatch, body):
    tmp_path, d, _few, many = corpus
    if body is not None:
        monkeypatch.setenv(FC.BODY, body)
    out = tmp_path / "out"
    for models in ([_uniform(64, 8)] * 17, [_uniform(33, 8)] * 17):
        res = _five(models, many, d / "t17.csv", [str(d / "x.seq")], out)
        assert res == [(1, _old_words(who)) for who in ENTRY_POINTS]
    assert not out.exists()


def test_a_bad_word_is_refused_by_each_entry_point_before_any_hip_call(corpus, monkeypatch):
    tmp_path, d, few, _many = corpus
    monkeypatch.setenv(FC.BODY, "fast")
    out = tmp_path / "out"
    # (this process has no device: a refusal with these words came before the first HIP call, which would have said so)
    for rc, msg in _five([_uniform(3, 8)] * 2, few, d / "t2.csv", [str(d / "x.seq")], out):
        assert rc == 1 and msg == BAD, msg
    assert not out.exists()
    # the earlier checks keep their place: a bad price is seen before the variable
    assert _posteriors_c([_uniform(3, 8)] * 2, [[0.0, 0.5], [0.0, 0.0]]) == 1 and "lt[0][1] = 0.5" in _err()
    assert _estep_c([_uniform(3, 8)] * 2, [[0.0, 0.5], [0.0, 0.0]]) == 1 and "lt[0][1] = 0.5" in _err()


@pytest.mark.parametrize("body", ["auto", "looped"])
def test_under_the_opt_in_the_widest_sets_pass_every_host_check_and_reach_the_device(corpus, monkeypatch, body):
    tmp_path, d, _few, many = corpus
    monkeypatch.setenv(FC.BODY, body)
    monkeypatch.setenv("ECOZ2_VQ_QUIET", "1")
    device = e.lib.e2vq_device_count() > 0
    out = tmp_path / "out"
    for rc, msg in _five([_uniform(64, 8)] * 17, many, d / "t17.csv", [str(d / "x.seq")], out):
        assert rc == 0 if device else (rc == 1 and "no HIP device" in msg), msg
    for models in ([_uniform(64, 8)] * 64, [_uniform(33, 8)] * 124):  # 4096 states in 64 slots; 124 slots, the most of the rows
        K = len(models)
        for rc in (_posteriors_c(models, np.full((K, K), -1.0)), _estep_c(models, np.full((K, K), -1.0))):
            assert rc == 0 if device else (rc == 1 and "no HIP device" in _err()), _err()
    # the other refusals keep their words under the opt-in
    assert _posteriors_c([_uniform(64, 8)] * 65, np.zeros((65, 65))) == 1 and "4160 states in all models (at most 4096)" in _err()
    monkeypatch.setenv(FC.ROUTE_C, "shared")
    assert _estep_c([_uniform(64, 8)] * 17, np.full((17, 17), -1.0)) == 1 and _err() == "ECOZ2_HMM_TRANS_EM_C=shared: lds or global"
    monkeypatch.setenv(FC.ROUTE_C, "lds")
    assert _estep_c([_uniform(1, 8)] * 150, np.full((150, 150), -1.0)) == 1
    assert "e2vq_hmm_transitions_estep: 150 classes of 150 states with the count table in LDS take" in _err()


def test_the_other_two_body_variables_are_never_read_by_these_calls(corpus, monkeypatch):
    tmp_path, d, few, many = corpus
    out = tmp_path / "out"
    for word in ("auto", "looped", "fast"):
        for name in FC.OTHER_BODIES:
            monkeypatch.setenv(name, word)
        # seventeen slots stay refused with the old words, and a word those variables would refuse passes unseen
        res = _five([_uniform(64, 8)] * 17, many, d / "t17.csv", [str(d / "x.seq")], out)
        assert res == [(1, _old_words(who)) for who in ENTRY_POINTS], word
    assert not out.exists()
    # and this variable is not read by the decoder or by the posteriors with one price
    for name in FC.OTHER_BODIES:
        monkeypatch.delenv(name)
    monkeypatch.setenv(FC.BODY, "auto")
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment_trans([_uniform(64, 8)] * 17, np.zeros(8, np.uint16), [0, 8], np.zeros((17, 17)))
    assert SLOTS17_DECODE in str(ei.value)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment_posteriors([_uniform(64, 8)] * 17, np.zeros(8, np.uint16), [0, 8], -1.0)
    assert SLOTS17 + "the posteriors have no looped body)" in str(ei.value)


def test_the_python_keywords_and_the_restored_environment(corpus, monkeypatch):
    tmp_path, d, few, many = corpus
    ok, sym = [_uniform(3, 8)] * 2, np.zeros(8, np.uint16)
    x = [str(d / "x.seq")]
    with pytest.raises(e.Ecoz2Error):
        hmm.transitions_estep(ok, sym, [0, 8], np.zeros((2, 2)), body="fast")
    assert _err() == BAD
    with pytest.raises(e.Ecoz2Error):
        hmm.train_transitions(ok, sym, [0, 8], body="fast")
    assert _err() == BAD
    with pytest.raises(e.Ecoz2Error):
        hmm.learn_transitions_files(few, x, tmp_path / "o.csv", -5.0, body="fast")
    assert _err() == BAD and not (tmp_path / "o.csv").exists()
    with pytest.raises(e.Ecoz2Error):
        hmm.segment_files(few, x, -5.0, csv=tmp_path / "o", class_transitions=d / "t2.csv", grammar_posteriors=True,
                          grammar_posteriors_body="fast")
    assert _err() == BAD and not (tmp_path / "o").exists()
    with pytest.raises(e.Ecoz2Error):
        with hmm.trans_fb_body("fast"):
            hmm.segment_trans_posteriors(ok, sym, [0, 8], np.zeros((2, 2)))
    assert _err() == BAD
    assert FC.BODY not in os.environ  # (the wrappers restore the environment)
    monkeypatch.setenv(FC.BODY, "resident")
    with pytest.raises(e.Ecoz2Error):
        hmm.transitions_estep(ok, sym, [0, 8], np.zeros((2, 2)), body="fast")
    assert os.environ[FC.BODY] == "resident"  # ... to what it was
    monkeypatch.delenv(FC.BODY)
    with pytest.raises(ValueError, match="grammar_posteriors_body needs grammar_posteriors=True"):
        hmm.segment_files(few, x, -5.0, class_transitions=d / "t2.csv", grammar_posteriors_body="auto")
    with pytest.raises(ValueError, match="grammar_posteriors_body needs grammar_posteriors=True"):
        hmm.segment_files(few, x, -5.0, posteriors=True, grammar_posteriors_body="auto")
    with pytest.raises(ValueError):  # (as before)
        hmm.segment_files(few, x, -5.0, class_transitions=d / "t2.csv", grammar_posteriors=True, grammar_body="auto")
    with pytest.raises(ValueError):  # (as before, whatever the new keyword says)
        hmm.segment_files(few, x, -5.0, class_transitions=d / "t2.csv", grammar_posteriors=True, grammar_body="auto",
                          grammar_posteriors_body="auto")
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.transitions_estep([_uniform(64, 8)] * 17, sym, [0, 8], np.zeros((17, 17)), body="resident")
    assert SLOTS17_ESTEP in str(ei.value)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment_files(many, x, -5.0, csv=tmp_path / "o", class_transitions=d / "t17.csv", grammar_posteriors=True)
    assert SLOTS17 in str(ei.value) and not (tmp_path / "o").exists()
    for fn in (hmm.transitions_estep, hmm.train_transitions, hmm.learn_transitions_files):
        assert inspect.signature(fn).parameters["body"].default is None
    assert inspect.signature(hmm.segment_files).parameters["grammar_posteriors_body"].default is None
    # an earlier test pins these parameters, so the array call takes the body through the context manager
    assert list(inspect.signature(hmm.segment_trans_posteriors).parameters) == ["models", "sym", "offs", "ln_trans", "device"]
    for fn in (hmm.segment_trans_posteriors, hmm.transitions_estep, hmm.segment_files):
        assert "there is no looped body" not in fn.__doc__ and "there is one body" not in fn.__doc__


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------
def _cli(cwd, *args):
    r = subprocess.run([EXE, "hmm", *args], cwd=cwd, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


SEGMENT = ["segment", "--models", "in/A.hmm", "in/B.hmm", "--sequences", "in/x.seq", "--switch-penalty", "-5", "-c", "out"]
NEEDS = "hmm segment: --grammar-posteriors-body <auto|resident|looped> needs --grammar-posteriors"
EM = ["transitions", "--em", "-m", "in/A.hmm", "in/B.hmm", "--switch-penalty", "-1", "-o", "out.csv", "--sequences", "in/x.seq"]


@pytest.mark.parametrize("args,needle", [
    (SEGMENT + ["--grammar-posteriors-body", "auto"], NEEDS),
    (SEGMENT + ["--class-transitions", "in/t2.csv", "--grammar-posteriors-body", "auto"], NEEDS),
    (SEGMENT + ["--posteriors", "--grammar-posteriors-body", "auto"], NEEDS),
    (SEGMENT + ["--class-transitions", "in/t2.csv", "--grammar-posteriors", "--grammar-posteriors-body", "fast"],
     "hmm segment --grammar-posteriors: --grammar-posteriors-body fast: auto, resident or looped"),
    (SEGMENT + ["--class-transitions", "in/t2.csv", "--grammar-posteriors", "--grammar-posteriors-body", ""],
     "hmm segment --grammar-posteriors: --grammar-posteriors-body : auto, resident or looped"),
    (SEGMENT + ["--class-transitions", "in/t2.csv", "--grammar-posteriors", "--grammar-posteriors-body"],
     "--grammar-posteriors-body needs a value"),
    # the refusals the earlier tests pin keep their words next to the new flag
    (SEGMENT + ["--class-transitions", "in/t2.csv", "--grammar-posteriors", "--grammar-posteriors-body", "auto", "--grammar-body", "auto"],
     "hmm segment: --grammar-posteriors has the resident body only: not with --grammar-body"),
    (SEGMENT + ["--class-transitions", "in/t2.csv", "--grammar-posteriors", "--grammar-posteriors-body", "auto", "--body", "auto"],
     "hmm segment: --grammar-posteriors has the resident body and whole recordings only: not with --continuous or --body"),
    (SEGMENT + ["--class-transitions", "in/t2.csv", "--grammar-posteriors", "--grammar-posteriors-body", "auto", "--continuous", "rec"],
     "hmm segment: --grammar-posteriors has the resident body and whole recordings only: not with --continuous or --body"),
    (EM + ["--body", "fast"], "hmm transitions --em: --body fast: auto, resident or looped"),
    (EM + ["--body", ""], "hmm transitions --em: --body : auto, resident or looped"),
    (EM + ["--body"], "--body needs a value"),
    (["transitions", "-m", "in/A.hmm", "in/B.hmm", "-o", "out.csv", "--body", "auto", "in/seg.csv"], "hmm transitions: --body needs --em"),
])
def test_cli_refusals_of_the_new_flags(corpus, args, needle):
    tmp_path, _d, _few, _many = corpus
    rc, out, err = _cli(tmp_path, *args)
    assert rc == 2 and needle in err, (rc, out, err)
    assert not (tmp_path / "out").exists() and not (tmp_path / "out.csv").exists()


@pytest.mark.parametrize("args,needle", [
    (["segment", "--class-transitions", "in/t17.csv", "--grammar-posteriors", "-c", "out"], SLOTS17_DECODE),
    (["segment", "--class-transitions", "in/t17.csv", "--grammar-posteriors", "--grammar-posteriors-body", "resident", "-c", "out"],
     SLOTS17_DECODE),
    (["transitions", "--em", "-o", "out.csv"], SLOTS17_ESTEP),
    (["transitions", "--em", "-o", "out.csv", "--body", "resident"], SLOTS17_ESTEP),
])
def test_cli_seventeen_slots_without_the_opt_in_exit_1_with_the_old_words(corpus, args, needle):
    tmp_path, _d, _few, _many = corpus
    rc, out, err = _cli(tmp_path, *args, "--models" if args[0] == "segment" else "-m", *[f"in/c{k:02d}.hmm" for k in range(17)],
                        "--sequences", "in/x.seq", "--switch-penalty", "-5")
    assert rc == 1 and needle in out, (rc, out, err)
    assert not (tmp_path / "out").exists() and not (tmp_path / "out.csv").exists()


def test_cli_under_the_flags_seventeen_slots_reach_the_device(corpus):
    tmp_path, _d, _few, _many = corpus
    device = e.lib.e2vq_device_count() > 0
    many = [f"in/c{k:02d}.hmm" for k in range(17)]
    for args in (["segment", "--models", *many, "--class-transitions", "in/t17.csv", "--grammar-posteriors",
                  "--grammar-posteriors-body", "auto", "-c", "out"],
                 ["transitions", "--em", "-m", *many, "-o", "out.csv", "--body", "auto", "-I", "1"]):
        rc, out, err = _cli(tmp_path, *args, "--sequences", "in/x.seq", "--switch-penalty", "-5")
        assert rc == 0 if device else (rc == 1 and "no HIP device" in out), (rc, out, err)


def test_usage_gains_the_two_flags_and_keeps_every_pinned_line(tmp_path):
    rc, _out, err = _cli(tmp_path, "segment")
    assert rc == 2
    assert ("                  [--grammar-body <auto|resident|looped>]\n"
            "                  [--grammar-posteriors-body <auto|resident|looped>]\n"
            "                  (--signals <.wav files|dirs>... | --predictors <.prd files|dirs>... | --sequences <.seq files|dirs>...)\n") in err
    assert "                  (--grammar-posteriors-body, with --grammar-posteriors: the kernel body of the posteriors under the prices,\n" in err
    em = ("  ecoz2 hmm transitions --em -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15] --switch-penalty <x>\n"
          "                  [--init <file.csv>] [--alpha 1] [-a val_auto] [-I max_iterations] -o <file.csv>\n"
          "                  --sequences <.seq>... | --predictors <.prd>... | --signals <.wav>...\n"
          "                  [--body <auto|resident|looped>]\n"
          "                  (the same prices by Baum-Welch from unlabelled recordings under the models; <file.csv>.em.csv: the iterations)\n"
          "                  (--body: the kernel body of the E-step -- resident takes at most 16 wave-slots of classes, looped any\n")
    assert em in err


# ---- exports ---------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_exported_and_the_headers_name_the_variable():
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    r = subprocess.run([nm, "-D", "--defined-only", os.path.join(CSRC, "libecoz2vq.so")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    names = set(line.split()[-1] for line in r.stdout.splitlines() if line.strip())
    for part in ("launch_loop_posteriors_trans_looped", "launch_trans_estep_looped", "posteriors_trans_looped_lds_bytes",
                 "trans_estep_looped_lds_bytes", "posteriors_trans_looped_layout", "trans_estep_looped_layout", "trans_fb_body",
                 "runs_looped",
                 *[f"{k}ILb{a}ELb{w}EE" for k in ("k_hmm_loop_posteriors_trans_looped", "k_hmm_trans_estep_looped") for a in (0, 1) for w in (0, 1)]):
        assert any(part in n for n in names), part
    # the resident bodies are still there, under their own names
    for part in ("28launch_loop_posteriors_transERK", "18launch_trans_estepERK", "k_hmm_loop_posteriors_transILb0ELb0EE",
                 "k_hmm_trans_estepILb1ELb1EE"):
        assert any(part in n for n in names), part
    header = open(os.path.join(ROOT, "include", "ecoz2_classify.h")).read()
    assert FC.BODY in header and BAD.replace("fast", "<v>") in header
    for name in ENTRY_POINTS:
        assert isinstance(getattr(e.lib, name), C._CFuncPtr) and name in header[header.index("The body.  " + FC.BODY):]
    for h in ("hmm_device.h", "hmm_host.h"):
        text = open(os.path.join(CSRC, h)).read()
        assert ("launch_trans_estep_looped" if h == "hmm_device.h" else FC.BODY) in text
