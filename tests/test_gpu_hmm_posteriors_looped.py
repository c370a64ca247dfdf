"""The looped body of `hmm segment --posteriors` on the GPU (ECOZ2_HMM_POSTERIOR_BODY): the raw bits of post
and ln P(O | loop), and status, against the restatement without its cap (tests/hmm_posterior_looped_cases.py) above 16
wave-slots under `auto` -- one class to a slot and twelve, a wave that serves three slots, the headline shape, a one-class slot
next to packed ones with a ragged last turn --; forced where the resident body runs, against that body's words too; the event
batch at 17 slots, in one call and one stream a launch; small forward-table budgets; with ln_switch = -inf the softmax of the
scorer's ln P; the file form and the CLI; and, with nothing set, the refusal of 17 slots."""
import os
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_class_loop_cases as loop_cases
from . import hmm_posterior_looped_cases as LC
from . import hmm_posterior_restatement as R
from .test_gpu_hmm_posteriors import SETS, _assert_equal, _bits, _positive_models

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
NINF = float("-inf")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in (LC.BODY, LC.CHUNK):
        monkeypatch.delenv(k, raising=False)


# ---- 1. above 16 slots under auto ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ls", LC.SWITCHES)
@pytest.mark.parametrize("name", list(LC.WIDE))
def test_above_sixteen_slots_auto_gives_the_restatements_bits(name, ls):
    models, sym, offs = LC.wide_case(name)
    got = hmm.segment_posteriors(models, sym, offs, ls, body="auto")
    _assert_equal(got, LC.wide_reference(name, ls), (name, ls))
    assert got["post"].shape == (offs[-1], len(models)) and got["status"].tolist() == [0] * len(LC.LENGTHS)
    assert hmm.segment_posteriors_last_kernel_ms() > 0.0


def test_above_sixteen_slots_looped_and_the_environment_say_the_same(monkeypatch):
    models, sym, offs = LC.wide_case("mixed")
    want = LC.wide_reference("mixed", -3.0)
    _assert_equal(hmm.segment_posteriors(models, sym, offs, -3.0, body="looped"), want, "looped")
    monkeypatch.setenv(LC.BODY, "auto")
    _assert_equal(hmm.segment_posteriors(models, sym, offs, -3.0), want, "environment")


# ---- 2. forced where the resident body runs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["leaning", "positive"])
@pytest.mark.parametrize("M", [8, 300])
@pytest.mark.parametrize("name", list(SETS))
def test_forced_looped_gives_the_resident_bodys_words(name, M, kind):
    Ns = SETS[name]
    assert Ns == LC.RESIDENT[name] and LC.looped_route(Ns)["a_lds"] == (name != "64x16")  # (both instantiations are run)
    models = loop_cases.leaning_models(len(Ns) + M, Ns, M) if kind == "leaning" else _positive_models(Ns, M, seed=len(Ns) + M)
    sym, offs = LC.pack(LC.streams(len(Ns) * 100 + M, M, K=len(Ns)))
    for ls in LC.SWITCHES:
        resident = hmm.segment_posteriors(models, sym, offs, ls)
        _assert_equal(hmm.segment_posteriors(models, sym, offs, ls, body="looped"), resident, ("resident", ls))
        _assert_equal(hmm.segment_posteriors(models, sym, offs, ls, body="auto"), resident, ("auto", ls))
        _assert_equal(resident, R.posteriors(models, sym, offs, ls), ("restatement", ls))


# ---- 3. the first event in frame order decides ---------------------------------------------------------------------------------
def test_the_event_batch_at_seventeen_slots(monkeypatch):
    streams, kinds = loop_cases.event_batch()
    sym, offs = LC.pack(streams)
    models = loop_cases.event_models("64x17")
    T, S, ls = loop_cases.EVENT_T, len(streams), loop_cases.EVENT_LN_SWITCH
    want = LC.posteriors(models, sym, offs, ls)
    monkeypatch.setenv(LC.BODY, "auto")
    # A batch of clean streams goes first: memory the allocator hands out again then holds posteriors, not zeros, and a failed
    # stream's rows are +0.0 only if the kernel writes every one of them (T K = 2210 entries by a workgroup of 1024 threads).
    clean = hmm.segment_posteriors(models, np.tile(sym[:T], S), offs, ls)
    assert clean["status"].tolist() == [0] * S and (clean["post"].sum(axis=1) > 0.99).all()
    got = hmm.segment_posteriors(models, sym, offs, ls)
    _assert_equal(got, want)
    # (the first event in frame order decides: (DEAD, M) is 1, (M, DEAD) is 2)
    assert got["status"].tolist() == [0] + [2] * 6 + [1] * 6 + [1, 2] * 3 == [loop_cases.event_status(k, "posteriors") for k in kinds]
    assert np.isfinite(got["log_prob"][0]) and (got["log_prob"][1:] == NINF).all()
    failed = got["post"][T:]
    assert failed.shape == ((S - 1) * T, 17) and not failed.any() and not np.signbit(failed).any()
    assert np.array_equal(_bits(clean["post"][:T]), _bits(got["post"][:T]))
    monkeypatch.setenv(LC.CHUNK, "1")  # one stream per launch: a0 of an event stream is not 0
    hmm.segment_posteriors(models, np.tile(sym[:T], S), offs, ls)
    _assert_equal(hmm.segment_posteriors(models, sym, offs, ls), want, "chunks")


# ---- 4. chunk budgets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["33x17", "5x193"])
def test_chunk_budgets_give_the_same_bits_at_seventeen_slots(name, monkeypatch):
    Ns, M = LC.WIDE[name]
    models = LC.wide_models(name)
    sym, offs = LC.pack(LC.streams(4, M, list(range(0, 100, 9)) + [101, 50], K=len(Ns)))  # 14 streams of 0 .. 101 frames
    ls = -3.0
    monkeypatch.setenv(LC.BODY, "auto")
    one = hmm.segment_posteriors(models, sym, offs, ls)
    _assert_equal(one, LC.posteriors(models, sym, offs, ls))
    for budget in ("1", str(8 * (sum(Ns) + 16) * 150)):  # one stream per launch; a few streams per launch
        monkeypatch.setenv(LC.CHUNK, budget)
        _assert_equal(hmm.segment_posteriors(models, sym, offs, ls), one, budget)


# ---- 5. without switching ------------------------------------------------------------------------------------------------------
def test_without_switching_the_rows_are_the_softmax_of_the_scorer_at_seventeen_slots():
    """as test_gpu_hmm_posteriors.py shows it below 17 slots: sw = 0, so post[t][k] = P(O | k) / sum_k' P(O | k') at every t.
    The derived bound of the posteriors at T <= 129, N = 33 is 4 (2 T + 1) (N + 32) 2^-53 = 7.5e-12; the logarithm and the
    exponential of the round trip add below 1e-12; the bound asserted is the existing test's."""
    Ns = (33,) * 17
    models = _positive_models(Ns, 32, seed=9)
    streams = LC.streams(2, 32, (1, 2, 64, 65, 129))
    sym, offs = LC.pack(streams)
    got = hmm.segment_posteriors(models, sym, offs, NINF, body="auto")
    lp = hmm.score(models, streams)["log_prob"]  # (S, K)
    assert got["status"].tolist() == [0] * len(streams)
    worst = 0.0
    for s in range(len(streams)):
        w = np.exp(lp[s] - lp[s].max())
        soft = w / w.sum()
        rows = got["post"][offs[s]:offs[s + 1]]
        worst = max(worst, float(np.max(np.abs(rows - soft[None, :]))))
        assert abs(got["log_prob"][s] - (lp[s].max() + np.log(w.sum()))) <= 1e-9 * max(1.0, abs(got["log_prob"][s]))
    print(f"33x17: worst |post - softmax| = {worst:.3e}")
    assert worst <= 1e-9


# ---- 6. the file form and the CLI ----------------------------------------------------------------------------------------------
def test_the_cli_and_the_file_form_at_seventeen_models(tmp_path):
    env = dict(os.environ)
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_GPUS", "ECOZ2_HMM_SEGMENT_BODY", "ECOZ2_HMM_SEGMENT_CHUNK_BYTES", LC.BODY, LC.CHUNK):
        env.pop(k, None)
    M, ls, T = 8, -3.0, 150
    Ns = (33,) * 17
    models = loop_cases.leaning_models(3, Ns, M)
    names = [f"c{k:02d}" for k in range(17)]  # (the order in which a directory of models is resolved)
    for c, m in zip(names, models):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)
    sym = loop_cases.run_stream(5, 17, M, T)
    e.formats.write_seq(str(tmp_path / "x.seq"), "_", M, sym)

    def run(*args, rc=0):
        r = subprocess.run([EXE, "hmm", "segment", "--models", "hmms", "--switch-penalty", str(ls), "--sequences", "x.seq", *args],
                           cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == rc, (r.stdout, r.stderr)
        return r.stdout

    run("-c", "plain")
    assert "the classes take 17 wave-slots" in run("-c", "no", "--posteriors", rc=1) and not (tmp_path / "no").exists()
    run("-c", "post", "--posteriors", "--frame-posteriors", "frames", "--body", "auto")
    rows = (tmp_path / "plain" / "x.csv").read_text().split("\n")
    want = (tmp_path / "post" / "x.csv").read_text().split("\n")
    frames = (tmp_path / "frames" / "x.csv").read_text().split("\n")
    # the first eight columns are the flag-less run's, byte for byte
    assert len(want) == len(rows) and want[0] == rows[0] + ",posterior,min_posterior"
    assert [",".join(r.split(",")[:8]) for r in want[1:-1]] == rows[1:-1] and want[-1] == ""
    # the new columns and the per-frame table: those computed from the array calls
    seg = hmm.segment(models, sym, [0, T], ls)
    post = hmm.segment_posteriors(models, sym, [0, T], ls, body="auto")
    _assert_equal(post, LC.posteriors(models, sym, [0, T], ls))
    g = lambda v: "%.17g" % v
    stats = R.segment_posteriors(seg["cls"], seg["entered"], post["post"])
    assert len(stats) == len(want) - 2 >= 2
    assert [r.split(",")[8:] for r in want[1:-1]] == [[g(a), g(b)] for a, b in stats]
    assert len(frames) == T + 2 and all(frames[t + 1].split(",")[3:] == [g(v) for v in post["post"][t]] for t in range(T))
    # the Python mirror of the file call
    files = [str(tmp_path / "hmms" / f"{c}.hmm") for c in names]
    hmm.segment_files(files, [str(tmp_path / "x.seq")], ls, csv=tmp_path / "py", posteriors=True, frame_posteriors=tmp_path / "py_frames",
                      body="auto")
    assert (tmp_path / "py" / "x.csv").read_text().split("\n") == want
    assert (tmp_path / "py_frames" / "x.csv").read_text().split("\n") == frames
    with pytest.raises(e.Ecoz2Error, match="17 wave-slots"):
        hmm.segment_files(files, [str(tmp_path / "x.seq")], ls, csv=tmp_path / "py2", posteriors=True)


# ---- 7. with nothing set -------------------------------------------------------------------------------------------------------
def test_with_nothing_set_seventeen_slots_are_still_refused():
    models, sym, offs = LC.wide_case("33x17")
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment_posteriors(models, sym, offs, -3.0)
    assert "the classes take 17 wave-slots of 64 lanes (at most 16: the posteriors have no looped body)" in str(ei.value)
