"""The looped body of `hmm align --posteriors` on the GPU (ECOZ2_HMM_ALIGN_POSTERIOR_BODY): every output of
e2vq_hmm_align_posteriors -- occ, post_path, w0, w1, w2, the host moments, the raw bits of ln P and the status -- against the
numpy restatement (tests/hmm_align_posterior_restatement.py, its slot bound lifted), no tolerance -- above 16 slots (a wave with
two and with three slots, A in global memory); the looped body forced below 17 slots, where it must also equal the resident
body's words; both routes of A forced; the lengths around 64 frames and T = the mandatory units; optional units; the order of
the events; batches under `auto`, whose launches are cut where the body changes; the E-step and `hmm.align` on the same
device; the refusals; the file form and the CLI under `auto`; and the default, which still refuses."""
import functools
import os
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_align_cases as cases
from . import hmm_align_posterior_looped_cases as LC
from . import hmm_align_posterior_restatement as PR
from .test_gpu_hmm_align_posteriors import FIELDS, _assert_equal, _bits, _pack, _path_and_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
NINF = float("-inf")
M = cases.M
ENV = (LC.BODY, "ECOZ2_HMM_EMBED_A", "ECOZ2_HMM_EMBED_CHUNK_BYTES", "ECOZ2_HMM_ALIGN_BODY")


@pytest.fixture(autouse=True)
def _setup(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(PR, "MAX_SLOTS", 64)  # (the restatement's arithmetic covers any slot count)


def _args(streams, transcripts, optionals=None, seed=1):
    """-> (the packed arguments, path_unit, ref): path and ref drawn as the resident tests draw them, 0xFFFF and a unit >= L
    among them"""
    args = _pack(streams, transcripts, optionals)
    path, ref = _path_and_ref(args, np.random.default_rng(seed))
    return args, path, ref


def _run(body, models, streams, transcripts, optionals=None, ls=0.0, seed=1):
    args, path, ref = _args(streams, transcripts, optionals, seed)
    return hmm.align_posteriors(models, *args, ls, path_unit=path, ref=ref, body=body)


def _want(models, streams, transcripts, optionals=None, ls=0.0, seed=1):
    args, path, ref = _args(streams, transcripts, optionals, seed)
    return PR.posteriors(models, *args, ls, path_unit=path, ref=ref)


def _opts(opt):
    return None if opt is None else [opt]


# ---- above 16 slots ----------------------------------------------------------------------------------------------------------------
ABOVE = {"64x17": (17, True), "33x20": (20, True), "64x6c_17u": (17, False), "33 slots": (33, True)}


@pytest.mark.parametrize("name", list(ABOVE))
def test_every_output_equals_the_restatement_above_sixteen_slots(name):
    models, units, opt, stream = LC.case(name)
    Ns = [len(m[0]) for m in models]
    slots, a_lds = ABOVE[name]
    assert PR.slots_of(models, units) == slots and len(stream) <= 400
    assert LC.looped_route(Ns, len(units), slots, sum(Ns[k] for k in units)) is a_lds
    for ls in (0.0, -3.0):
        got, want = _run("auto", models, [stream], [units], _opts(opt), ls), _want(models, [stream], [units], _opts(opt), ls)
        _assert_equal(got, want, (name, ls))
        assert got["status"].tolist() == [0] and np.isfinite(got["log_prob"][0])
    _assert_equal(_run("looped", models, [stream], [units], _opts(opt), -3.0), got, (name, "looped"))
    assert hmm.align_posteriors_last_kernel_ms() > 0.0


# ---- the looped body forced at 16 slots and below: the resident body's words ---------------------------------------------------------
@pytest.mark.parametrize("name", ["5x13", "mixed", "64x16", "1x3c_200u", "1x3c_201u_opt", "1_64_1", "mixed_M1024", "small_M65536"])
def test_the_forced_looped_body_gives_the_resident_bodys_words(name):
    models, units, opt, stream = LC.case(name)
    assert PR.slots_of(models, units) <= 16
    want = _want(models, [stream], [units], _opts(opt), -1.0)
    resident = _run("resident", models, [stream], [units], _opts(opt), -1.0)
    looped = _run("looped", models, [stream], [units], _opts(opt), -1.0)
    _assert_equal(looped, want, name)
    _assert_equal(looped, resident, (name, "resident"))
    assert want["status"].tolist() == [0]


# ---- forced routes of A ------------------------------------------------------------------------------------------------------------
def test_both_forced_routes_of_a_give_the_same_bits(monkeypatch):
    models, units, _opt, stream = LC.case("33x20")
    want = _want(models, [stream], [units], None, -1.0)
    for a in ("lds", "global"):
        monkeypatch.setenv("ECOZ2_HMM_EMBED_A", a)
        _assert_equal(_run("auto", models, [stream], [units], None, -1.0), want, a)
    # a forced layout that does not fit is refused on the host: A of six 64-state classes takes 195 KB
    models, units, _opt, stream = LC.case("64x6c_17u")
    monkeypatch.setenv("ECOZ2_HMM_EMBED_A", "lds")
    need = LC.align_post_looped_lds_bytes(17, 17, 17 * 64, 6 * 64 * 65, True)
    with pytest.raises(Exception, match=rf"17 units of sum N = 1088 states in 17 wave-slots and A in LDS take {need} bytes of LDS "
                                        r"\(at most 163840\)"):
        _run("auto", models, [stream], [units])


# ---- the lengths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 10, 63, 64, 65, 129])
def test_lengths_around_sixty_four_frames_and_at_the_mandatory_units(T):
    """T = 10 with every other unit optional: as many frames as mandatory units.  T = 1 has no path: status 1, every output
    0.0, no moments."""
    models, units, _opt, stream = LC.case("33x20")
    opt = np.array([l % 2 for l in range(20)], np.uint8) if T == 10 else None
    got, want = _run("auto", models, [stream[:T]], [units], _opts(opt), -0.5), _want(models, [stream[:T]], [units], _opts(opt), -0.5)
    _assert_equal(got, want, T)
    assert got["status"].tolist() == [1 if T == 1 else 0]
    if T == 1:
        assert not got["occ"][0].any() and not got["post_path"].any() and got["log_prob"][0] == NINF
        assert not any(got[w].any() for w in ("w0", "w1", "w2", "present")) and np.isnan(got["begin_mean"]).all()


# ---- optional units ----------------------------------------------------------------------------------------------------------------
def test_optional_units_at_seventeen_slots():
    """Every third unit optional, the first and the last among them: 0, 3, 6, 9, 12 and, since 16 is no multiple of 3, 16 in
    place of 15.  A path may pass over an optional unit, so its presence lies in [0, 1] and below 1 somewhere; the presence of a
    mandatory unit is 1 in exact arithmetic and here a sum of T rounded terms, held to the 1e-12 the CPU file asks of it."""
    models, units, _none, stream = LC.case("64x17")
    opt = np.zeros(17, np.uint8)
    opt[[0, 3, 6, 9, 12, 16]] = 1
    got, want = _run("auto", models, [stream], [units], [opt], -1.0), _want(models, [stream], [units], [opt], -1.0)
    _assert_equal(got, want)
    assert got["status"].tolist() == [0]
    p = got["present"]
    print("present of the optional units", p[opt == 1], "largest |present - 1| of the mandatory ones", np.abs(p[opt == 0] - 1.0).max())
    assert (p[opt == 1] >= 0.0).all() and (p[opt == 1] <= 1.0).all() and (p < 1.0).any()
    assert (np.abs(p[opt == 0] - 1.0) < 1e-12).all()
    assert np.abs(got["occ"][0].sum(axis=1) - 1.0).max() < 1e-12


# ---- the events --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _events():
    models = cases.event_models()
    streams, transcripts, optionals, kinds = cases.event_batch()
    return models, streams, transcripts, optionals, kinds, _want(models, streams, transcripts, optionals, -1.0)


@pytest.mark.parametrize("chunk_bytes", [None, "1"])
def test_the_status_events_and_a_clean_stream_among_them_in_the_looped_body(chunk_bytes, monkeypatch):
    if chunk_bytes:
        monkeypatch.setenv("ECOZ2_HMM_EMBED_CHUNK_BYTES", chunk_bytes)  # a launch per stream
    models, streams, transcripts, optionals, kinds, want = _events()
    got = _run("looped", models, streams, transcripts, optionals, -1.0)
    _assert_equal(got, want, chunk_bytes)
    code = {"clean": 0, "M": 2, "dead": 1, "dead_M": 1, "M_dead": 2}
    assert got["status"].tolist() == [code[k] for k in kinds]
    T, L = cases.EVENT_T, 4
    for s, k in enumerate(kinds):
        if k != "clean":  # every entry of the stream is 0.0, ln P is -inf
            assert not got["occ"][s].any() and not got["post_path"][s * T:(s + 1) * T].any() and got["log_prob"][s] == NINF
            assert not any(got[w][s * L:(s + 1) * L].any() for w in ("w0", "w1", "w2"))
            assert np.isnan(got["begin_mean"][s * L:(s + 1) * L]).all()
    # the clean stream alone: its neighbours change none of its bits
    _all, path, ref = _args(streams, transcripts, optionals)
    alone = hmm.align_posteriors(models, *_pack(streams[:1], transcripts[:1], optionals[:1]), -1.0, path_unit=path[:T], ref=ref[:L],
                                 body="looped")
    for k in FIELDS:
        n = 1 if k == "log_prob" else T if k == "post_path" else L
        assert np.array_equal(_bits(alone[k]), _bits(got[k][:n])), k
    assert alone["status"].tolist() == [0] and np.array_equal(_bits(alone["occ"][0]), _bits(got["occ"][0]))


# ---- batches under auto ------------------------------------------------------------------------------------------------------------
def test_the_random_batch_under_auto():
    """Seed 24, L from 1 .. 40 (the batch test_gpu_hmm_align_shapes.py documents): 5 of the 40 streams take 17 to 20 slots and lie
    between resident ones, so the launch is cut at every change of the body; every stream has status 0."""
    models, streams, transcripts, optionals = cases.random_batch(LC.RANDOM_SEED, LC.RANDOM_MAX_L)
    slots = [PR.slots_of(models, u) for u in transcripts]
    wide = [s > 16 for s in slots]
    assert len(streams) == 40 and sum(wide) == 5 and all(17 <= s <= 20 for s in slots if s > 16)
    assert sum(a != b for a, b in zip(wide, wide[1:])) >= 4 and not wide[0] and not wide[-1]
    got, want = _run("auto", models, streams, transcripts, optionals, -1.0), _want(models, streams, transcripts, optionals, -1.0)
    _assert_equal(got, want, "auto")
    assert got["status"].tolist() == [0] * 40


def test_unlike_streams_and_a_seventeen_slot_stream_in_one_call():
    models, streams, transcripts, optionals = cases.unlike_streams()
    _m17, u17, s17 = cases.packing("64x17")
    # the 64-state classes 3 .. 5 stand in for the packing's three: the 17-slot stream goes between the resident ones
    streams = streams[:2] + [s17[:150]] + streams[2:]
    transcripts = transcripts[:2] + [u17 + 3] + transcripts[2:]
    optionals = optionals[:2] + [np.zeros(17, np.uint8)] + optionals[2:]
    assert [PR.slots_of(models, u) for u in transcripts] == [1, 2, 17, 8, 3]
    got, want = _run("auto", models, streams, transcripts, optionals, -1.0), _want(models, streams, transcripts, optionals, -1.0)
    _assert_equal(got, want)
    assert got["status"].tolist() == [0] * 5
    with pytest.raises(Exception, match=r"stream 2: the units take 17 wave-slots"):
        _run("resident", models, streams, transcripts, optionals, -1.0)


# ---- against the E-step and the alignment on the same device -------------------------------------------------------------------------
def test_log_prob_and_status_are_the_embedded_esteps_bits():
    m17, u17, s17 = cases.packing("64x17")
    for models, streams, transcripts, optionals in ((m17, [s17], [u17], None), (cases.event_models(),) + cases.event_batch()[:3]):
        args = _pack(streams, transcripts, optionals)
        a = hmm.align_posteriors(models, *args, -1.0, occupancy=False, body="auto")
        b = hmm.embedded_estep(models, *args, -1.0, body="auto")
        assert "occ" not in a and np.array_equal(a["status"], b["status"]) and np.array_equal(_bits(a["log_prob"]), _bits(b["log_prob"]))
        c = hmm.align_posteriors(models, *args, -1.0, occupancy=False, body="looped")
        assert np.array_equal(c["status"], b["status"]) and np.array_equal(_bits(c["log_prob"]), _bits(b["log_prob"]))


def test_the_path_of_hmm_align_reads_its_own_column_of_the_occupancy():
    models, units, stream = cases.packing("64x17")
    T, L = len(stream), len(units)
    args = (stream, np.array([0, T]), units, np.array([0, L]), None)
    al = hmm.align(models, *args, -1.0)
    assert al["status"].tolist() == [0]
    ref = np.where(al["begin"] < 0, 0, al["begin"])
    got = hmm.align_posteriors(models, *args, -1.0, path_unit=al["unit"], ref=ref, body="auto")
    _assert_equal(got, PR.posteriors(models, *args, -1.0, path_unit=al["unit"], ref=ref))
    want = got["occ"][0][np.arange(T), al["unit"]]
    assert np.array_equal(_bits(got["post_path"]), _bits(want)) and (want > 0).all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_the_refusals_come_before_the_device(monkeypatch):
    N, L, slots, sumN = LC.too_large()
    need = LC.align_post_looped_lds_bytes(L, slots, sumN, 0, False)
    uni = cases.uniform_model(N)
    with pytest.raises(Exception, match=rf"stream 0: {L} units of sum N = {sumN} states in {slots} wave-slots do not fit in LDS "
                                        rf"\({need} of {LC.SEG_LDS_BYTES} bytes\)"):
        hmm.align_posteriors([uni], np.zeros(8, np.uint16), [0, 8], [0] * L, [0, L], body="auto")
    models, units, stream = cases.packing("64x17")
    with pytest.raises(Exception, match="ECOZ2_HMM_ALIGN_POSTERIOR_BODY=fast: auto, resident or looped"):
        hmm.align_posteriors(models, stream, [0, len(stream)], units, [0, 17], body="fast")
    with pytest.raises(Exception, match=r"stream 0: the units take 17 wave-slots of 64 lanes \(at most 16: the alignment posteriors have a "
                                        r"resident body only\)"):
        hmm.align_posteriors(models, stream, [0, len(stream)], units, [0, 17])


# ---- the file form and the CLI -----------------------------------------------------------------------------------------------------
def test_the_file_form_and_the_cli_score_thirty_five_slots_under_auto(tmp_path):
    env = dict(os.environ)
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_GPUS", "ECOZ2_VQ_QUIET") + ENV:
        env.pop(k, None)
    ls = -1.0
    names = ["a", "bg"]
    models = cases.small_models(seed=17, Ns=(64, 2), zeros=0.0)
    for c, m in zip(names, models):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)
    stream = np.random.default_rng(18).integers(0, M, 90).astype(np.uint16)
    e.formats.write_seq(str(tmp_path / "x.seq"), "_", M, stream)
    (tmp_path / "x.csv").write_text("class\n" + "a\n" * 17)
    units = np.array([1] + [0, 1] * 17, np.int32)  # the filler around and between the 17 labels
    opt = (units == 1).astype(np.uint8)
    T, L = len(stream), len(units)
    assert PR.slots_of(models, units) == 35
    files = [str(tmp_path / "hmms" / f"{c}.hmm") for c in names]
    seq, lab = [str(tmp_path / "x.seq")], [str(tmp_path / "x.csv")]
    with pytest.raises(e.Ecoz2Error, match="the alignment posteriors have a resident body only"):
        hmm.align_files(files, seq, lab, ls, filler="bg", csv=tmp_path / "no.csv", posteriors=True)
    assert not (tmp_path / "no.csv").exists()
    hmm.align_files(files, seq, lab, ls, filler="bg", csv=tmp_path / "py.csv", posteriors=True, frame_posteriors=tmp_path / "pyframes",
                    body="auto")
    # what the array form computes: the alignment's path and begin, then the posteriors
    args = (stream, np.array([0, T]), units, np.array([0, L]), opt)
    al = hmm.align(models, *args, ls)
    assert al["status"].tolist() == [0]
    ref = np.where(al["begin"] < 0, 0, al["begin"])
    want = hmm.align_posteriors(models, *args, ls, path_unit=al["unit"], ref=ref, body="auto")
    _assert_equal(want, PR.posteriors(models, *args, ls, path_unit=al["unit"], ref=ref))
    assert want["status"].tolist() == [0]
    rows = (tmp_path / "py.csv").read_text().splitlines()
    assert rows[0].split(",")[7:] == ["posterior", "min_posterior", "p_present", "begin_mean_frame", "begin_sd_frames"]
    visited = [l for l in range(L) if al["begin"][l] >= 0]
    assert len(rows) == 1 + len(visited)
    for row, l in zip(rows[1:], visited):
        b, en = int(al["begin"][l]), int(al["end"][l])
        total = 0.0
        for v in want["post_path"][b:en]:
            total = total + float(v)
        tail = [total / float(en - b), float(want["post_path"][b:en].min()), want["present"][l], want["begin_mean"][l], want["begin_sd"][l]]
        assert row.split(",")[:4] == [str(l), names[units[l]], str(b), str(en)]
        assert row.split(",")[7:] == ["%.17g" % v for v in tail], (l, row)
    frames = (tmp_path / "pyframes" / "x.csv").read_text().splitlines()
    assert frames[0] == "frame,begin_s,unit,class,posterior" and len(frames) == 1 + T
    assert [x.split(",")[2:] for x in frames[1:]] == [[str(int(al["unit"][t])), names[units[al["unit"][t]]], "%.17g" % want["post_path"][t]]
                                                      for t in range(T)]
    # the CLI writes the same bytes, and prints the p= lines
    common = [EXE, "hmm", "align", "--models", "hmms", "--labels", "x.csv", "--filler", "bg", "--switch-penalty", str(ls)]
    run = lambda *a: subprocess.run([*common, *a, "--sequences", "x.seq"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    r = run("-c", "cli.csv", "--posteriors", "--frame-posteriors", "frames", "--body", "auto")
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert (tmp_path / "cli.csv").read_text() == (tmp_path / "py.csv").read_text()
    assert (tmp_path / "frames" / "x.csv").read_text() == (tmp_path / "pyframes" / "x.csv").read_text()
    assert len([x for x in r.stdout.splitlines() if " p=" in x]) == len(visited)
    r = run("-c", "no.csv", "--posteriors")
    assert r.returncode == 1 and "the alignment posteriors have a resident body only" in r.stdout and not (tmp_path / "no.csv").exists()
    r = run("-c", "no.csv", "--body", "auto")
    assert r.returncode == 2 and "--body <auto|resident|looped> needs --posteriors" in r.stderr and not (tmp_path / "no.csv").exists()


# ---- the default -------------------------------------------------------------------------------------------------------------------
def test_with_nothing_set_seventeen_slots_are_still_refused():
    models, units, stream = cases.packing("64x17")
    with pytest.raises(Exception, match=r"stream 0: the units take 17 wave-slots of 64 lanes \(at most 16: the alignment posteriors have a "
                                        r"resident body only\)"):
        _run(None, models, [stream], [units])
