"""The looped bodies of the forward-backward passes under class-to-class prices on the GPU (DESIGN.md 4.8.13 and 4.8.14,
ECOZ2_HMM_TRANS_FB_BODY): above 16 wave-slots the raw bits of post, of every limb and both counters of the count table, of
ln P and the status against the numpy restatements, which have no slot cap; below the cap the looped bodies forced against the
resident ones at every placement of A, w and C; events between clean streams; a small table budget; a training on planted
data; the files and the CLI; what still refuses 17 slots.  No tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_class_loop_cases as loop_cases
from . import hmm_trans_fb_looped_cases as FC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
POST_KEYS = ("post", "log_prob", "status")
ESTEP_KEYS = ("acc", "log_prob", "status")
SLOTS17 = "the classes take 17 wave-slots of 64 lanes (at most 16: "


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in (FC.BODY, FC.CHUNK, FC.ROUTE_C, *FC.OTHER_BODIES):
        monkeypatch.delenv(k, raising=False)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _assert_equal(got, want, keys, note=None):
    for key in keys:
        a, b = _bits(got[key]), _bits(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (
            key, note, np.flatnonzero(a.ravel() != b.ravel())[:5] if a.shape == b.shape else (a.shape, b.shape))


def _posteriors(models, sym, offs, lt, body):
    with hmm.trans_fb_body(body):
        return hmm.segment_trans_posteriors(models, sym, offs, lt)


# ---- 1. every wide row -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", ["auto", "looped"])
@pytest.mark.parametrize("name", list(FC.WIDE))
def test_the_wide_rows_equal_the_restatements(name, body):
    models, sym, offs, lt = FC.wide_case(name)
    _assert_equal(_posteriors(models, sym, offs, lt, body), FC.wide_posteriors(name), POST_KEYS, (name, body))
    assert hmm.segment_trans_posteriors_last_kernel_ms() > 0.0
    _assert_equal(hmm.transitions_estep(models, sym, offs, lt, body=body), FC.wide_estep(name), ESTEP_KEYS, (name, body))
    assert hmm.transitions_estep_last_kernel_ms() > 0.0


# ---- 2. forced where the resident bodies run: their words ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(loop_cases.TRANS_POSTERIORS_SHAPES))
def test_below_the_cap_the_looped_posteriors_are_the_resident_bodys(name):
    models, stream, lt = loop_cases.trans_posteriors_shape(name)
    offs = [0, len(stream)]
    want = _posteriors(models, stream, offs, lt, "resident")
    assert want["status"].tolist() == [0]
    _assert_equal(_posteriors(models, stream, offs, lt, "looped"), want, POST_KEYS, name)
    _assert_equal(_posteriors(models, stream, offs, lt, "auto"), want, POST_KEYS, name)  # (resident below the cap)


@pytest.mark.parametrize("name", list(loop_cases.GRAMMAR_SHAPES))
def test_below_the_cap_the_looped_e_step_is_the_resident_bodys(name):
    models, stream, lt = loop_cases.grammar_shape(name)
    offs = [0, len(stream)]
    want = hmm.transitions_estep(models, stream, offs, lt, body="resident")
    assert want["status"].tolist() == [0] and np.count_nonzero(want["acc"]) > 2
    _assert_equal(hmm.transitions_estep(models, stream, offs, lt, body="looped"), want, ESTEP_KEYS, name)


def test_the_count_table_in_global_memory_at_64x17(monkeypatch):
    models, sym, offs, lt = FC.wide_case("64x17")
    monkeypatch.setenv(FC.ROUTE_C, "global")
    for body in ("auto", "looped"):
        _assert_equal(hmm.transitions_estep(models, sym, offs, lt, body=body), FC.wide_estep("64x17"), ESTEP_KEYS, body)
    monkeypatch.setenv(FC.ROUTE_C, "lds")
    _assert_equal(hmm.transitions_estep(models, sym, offs, lt, body="auto"), FC.wide_estep("64x17"), ESTEP_KEYS, "lds")


# ---- 3. events ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.EVENT_ROWS)
def test_events_fail_alone_and_leave_their_neighbours_untouched(name):
    models, sym, offs, lt, kinds = FC.event_case(name)
    K = len(models)
    want_p, want_e = FC.event_posteriors(name), FC.event_estep(name)
    status = [{"clean": 0, "M": 2, "dead": 1}[k] for k in kinds]
    for body in ("auto", "looped"):
        got = _posteriors(models, sym, offs, lt, body)
        assert got["status"].tolist() == status
        _assert_equal(got, want_p, POST_KEYS, (name, body))
        for s, k in enumerate(kinds):
            rows = got["post"][offs[s]:offs[s + 1]]
            assert (rows == 0.0).all() if k != "clean" else abs(rows.sum() - FC.EVENT_T) < 1e-6
        got = hmm.transitions_estep(models, sym, offs, lt, body=body)
        _assert_equal(got, want_e, ESTEP_KEYS, (name, body))
        assert got["acc"][2 * K * K:].tolist() == [kinds.count("clean"), len(kinds) - kinds.count("clean")]
    # nothing is added to C by the failed streams but the second counter: the clean streams alone give the same limbs
    clean = [s for s, k in enumerate(kinds) if k == "clean"]
    csym, coffs = FC.pack([sym[offs[s]:offs[s + 1]] for s in clean])
    alone = hmm.transitions_estep(models, csym, coffs, lt, body="auto")
    assert np.array_equal(alone["acc"][:2 * K * K], got["acc"][:2 * K * K]) and alone["acc"][2 * K * K:].tolist() == [len(clean), 0]


# ---- 4. a small table budget: several launches, no bit changes ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["64x17", "5x204", "33x33"])
def test_chunked_launches_change_no_bit(name, monkeypatch):
    models, sym, offs, lt = FC.wide_case(name)
    Ns, _M = FC.WIDE[name]
    # room for 130 frames of the forward table (8 (sum N + 16) bytes a frame): 129 alone, 63 + 64, 65, 0 + 1 + 2 ...
    monkeypatch.setenv(FC.CHUNK, str(130 * 8 * (sum(Ns) + 16)))
    _assert_equal(_posteriors(models, sym, offs, lt, "auto"), FC.wide_posteriors(name), POST_KEYS, name)
    _assert_equal(hmm.transitions_estep(models, sym, offs, lt, body="auto"), FC.wide_estep(name), ESTEP_KEYS, name)
    monkeypatch.setenv(FC.CHUNK, "1")  # a stream a launch
    _assert_equal(_posteriors(models, sym, offs, lt, "auto"), FC.wide_posteriors(name), POST_KEYS, name)
    _assert_equal(hmm.transitions_estep(models, sym, offs, lt, body="auto"), FC.wide_estep(name), ESTEP_KEYS, name)


# ---- 5. a training -----------------------------------------------------------------------------------------------------------------
def test_three_iterations_on_planted_data_equal_the_restatements_loop():
    models, sym, offs = FC.train_case()
    want, whist = FC.train_reference()
    seen = []
    kw = dict(FC.TRAIN_KW)
    got, hist = hmm.train_transitions(models, sym, offs, None, callback=lambda v, x: seen.append(x), body="auto", **kw)
    print("L per E-step:", list(hist))
    assert len(hist) == len(whist) == FC.TRAIN_ITERATIONS and np.array_equal(_bits(hist), _bits(np.array(whist)))
    assert np.array_equal(_bits(got), _bits(want))
    assert seen == list(whist) and hist[0] <= hist[1] <= hist[2]
    with pytest.raises(e.Ecoz2Error) as ei:  # without the opt-in the refusal stands
        hmm.train_transitions(models, sym, offs, None, **kw)
    assert SLOTS17 + "the E-step of the class transitions has no looped body)" in str(ei.value)


# ---- 6. the files and the CLI ------------------------------------------------------------------------------------------------------
def test_files_and_cli_at_seventeen_classes_of_64_states(tmp_path):
    env = dict(os.environ)
    for k in (FC.BODY, FC.CHUNK, FC.ROUTE_C, *FC.OTHER_BODIES, "ECOZ2_VQ_QUIET"):
        env.pop(k, None)
    Ns, M = FC.WIDE["64x17"]
    models, sym, offs = FC.train_case()
    names = [f"c{k:02d}" for k in range(len(Ns))]
    files = []
    for c, m in zip(names, models):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)
        files.append(str(tmp_path / "hmms" / f"{c}.hmm"))
    seqs = []
    for s in range(len(offs) - 1):
        seqs.append(str(tmp_path / f"s{s}.seq"))
        e.formats.write_seq(seqs[-1], "c00", M, sym[offs[s]:offs[s + 1]])
    lt = loop_cases.forbidding_prices(FC.PRICE_SEED, len(Ns))
    hmm.write_class_transitions(tmp_path / "t.csv", names, lt)

    def cli(*args):
        r = subprocess.run([EXE, "hmm", *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        return r.returncode, r.stdout, r.stderr

    # without the flags the old refusals hold and nothing is written
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment_files(files, seqs[:2], -1.0, csv=tmp_path / "no", class_transitions=tmp_path / "t.csv", grammar_posteriors=True,
                          frame_posteriors=tmp_path / "nof")
    assert SLOTS17 in str(ei.value)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.learn_transitions_files(files, seqs, tmp_path / "no.csv", -1.0, max_iterations=2)
    assert SLOTS17 + "the E-step of the class transitions has no looped body)" in str(ei.value)
    rc, out, _err = cli("segment", "--models", "hmms", "--sequences", *seqs[:2], "--switch-penalty", "-1", "--class-transitions", "t.csv",
                        "--grammar-posteriors", "-c", "no", "--frame-posteriors", "nof")
    assert rc == 1 and SLOTS17 in out
    rc, out, _err = cli("transitions", "--em", "-m", "hmms", "--sequences", *seqs, "--switch-penalty", "-1", "-o", "no.csv", "-I", "2")
    assert rc == 1 and SLOTS17 in out
    for p in ("no", "nof", "no.csv", "no.csv.em.csv"):
        assert not (tmp_path / p).exists(), p

    # the posteriors: the Python keyword and the CLI flag write the same bytes
    hmm.segment_files(files, seqs[:2], -1.0, csv=tmp_path / "py", class_transitions=tmp_path / "t.csv", grammar_posteriors=True,
                      frame_posteriors=tmp_path / "pyf", grammar_posteriors_body="auto")
    rc, out, err = cli("segment", "--models", "hmms", "--sequences", *seqs[:2], "--switch-penalty", "-1", "--class-transitions", "t.csv",
                       "--grammar-posteriors", "--grammar-posteriors-body", "auto", "-c", "cli", "--frame-posteriors", "clif")
    assert rc == 0, (out, err)
    # ... and the segment columns are those of the decoder under --grammar-body auto, without posteriors
    rc, out, err = cli("segment", "--models", "hmms", "--sequences", *seqs[:2], "--switch-penalty", "-1", "--class-transitions", "t.csv",
                       "--grammar-body", "auto", "-c", "dec")
    assert rc == 0, (out, err)
    for s in ("s0", "s1"):
        rows = (tmp_path / "py" / f"{s}.csv").read_bytes()
        assert rows == (tmp_path / "cli" / f"{s}.csv").read_bytes() and len(rows.split(b"\n")) > 4
        assert (tmp_path / "pyf" / f"{s}.csv").read_bytes() == (tmp_path / "clif" / f"{s}.csv").read_bytes()
        with_p = [r.split(",") for r in rows.decode().split("\n")]
        plain = [r.split(",") for r in (tmp_path / "dec" / f"{s}.csv").read_text().split("\n")]
        assert len(with_p) == len(plain) and with_p[0][-2:] == ["posterior", "min_posterior"]
        assert [r[:8] for r in with_p if len(r) > 1] == [r[:8] for r in plain if len(r) > 1]
    # the per-frame table holds the posteriors of the array call
    frames = (tmp_path / "pyf" / "s0.csv").read_text().split("\n")
    with hmm.trans_fb_body("auto"):
        want = hmm.segment_trans_posteriors(models, sym[offs[0]:offs[1]], [0, int(offs[1] - offs[0])], lt + -1.0)
    assert frames[0].split(",")[3:] == names and len(frames) == FC.TRAIN_T + 2
    assert [r.split(",")[3:] for r in frames[1:-1]] == [["%.17g" % v for v in row] for row in want["post"]]

    # the training: the Python keyword and the CLI flag write a file that --class-transitions reads
    hmm.learn_transitions_files(files, seqs, tmp_path / "em.csv", -1.0, alpha=0.0, val_auto=-1e300, max_iterations=FC.TRAIN_ITERATIONS,
                                body="auto")
    want, whist = FC.train_reference()
    assert np.array_equal(_bits(hmm.read_class_transitions(tmp_path / "em.csv", names)), _bits(want))
    g = lambda v: "%.17g" % v
    assert (tmp_path / "em.csv.em.csv").read_text() == "iteration,sum_log_prob,streams_used,streams_skipped\n" + "".join(
        f"{i},{g(v)},{FC.TRAIN_STREAMS},0\n" for i, v in enumerate(whist))
    rc, out, err = cli("transitions", "--em", "-m", "hmms", "--sequences", *seqs, "--switch-penalty", "-1", "--alpha", "0", "-a", "-1e300",
                       "-I", str(FC.TRAIN_ITERATIONS), "--body", "auto", "-o", "em2.csv")
    assert rc == 0 and f"{FC.TRAIN_ITERATIONS} E-step(s); em2.csv saved" in out, (out, err)
    assert (tmp_path / "em2.csv").read_bytes() == (tmp_path / "em.csv").read_bytes()
    rc, out, err = cli("segment", "--models", "hmms", "--sequences", seqs[0], "--switch-penalty", "-1", "--class-transitions", "em.csv",
                       "--grammar-body", "auto", "-c", "seg")
    assert rc == 0 and len((tmp_path / "seg" / "s0.csv").read_text().split("\n")) > 4, (out, err)
