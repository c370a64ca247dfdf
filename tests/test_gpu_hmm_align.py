"""`hmm align` on the GPU: unit, state, entered, begin, end, the raw bits of score and ln P*, and status
against the numpy restatement (tests/hmm_align_restatement.py) at the smallest shape that reaches each code path of
k_hmm_align -- packed and one-unit slots, 16 slots, the looped body with one and with two slots to a wave, the looped body
forced on a resident shape --; the lengths around the 64-symbol hand-out and around T = L; optional units at both ends and
between all units, with one stream on which passing over them wins and one on which it does not; L = 1 against hmm.viterbi;
a batch in one launch and in a launch per stream; status 2 inside a batch; symbols in a device tensor; the file form and the
CLI against the CSV the test formats from the restatement's result."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_align_cases as cases
from . import hmm_align_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
NINF = float("-inf")
KEYS = ("unit", "state", "entered", "score", "begin", "end", "log_prob", "status")
M = cases.M


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _assert_equal(got, want, note=None, keys=KEYS):
    for key in keys:
        a, b = _bits(got[key]), _bits(want[key])
        assert a.dtype == b.dtype and np.array_equal(a, b), (key, note, np.flatnonzero(a != b)[:5] if a.shape == b.shape else (a.shape, b.shape))


def _both(models, streams, transcripts, optionals=None, ls=0.0):
    """(the GPU's result, the restatement's) of streams aligned to their transcripts"""
    sym, offs = hmm._pack(streams)
    units = np.concatenate(transcripts).astype(np.int32)
    unit_offs = np.concatenate([[0], np.cumsum([len(u) for u in transcripts])]).astype(np.int64)
    opt = None if optionals is None else np.concatenate(optionals).astype(np.uint8)
    got = hmm.align(models, sym, offs, units, unit_offs, opt, ls)
    want = R.align(models, sym, offs, units, unit_offs, opt, ls)
    for s, us in enumerate(got["units"]):
        a, b, ua, ub = offs[s], offs[s + 1], unit_offs[s], unit_offs[s + 1]
        ref = R.units_of(units[ua:ub], want["begin"][ua:ub], want["end"][ua:ub], want["score"][a:b], ls)
        assert [(g["unit"], g["cls"], g["begin"], g["end"]) for g in us] == [r[:4] for r in ref]
        assert np.array_equal(_bits(np.array([g["score"] for g in us])), _bits(np.array([r[4] for r in ref])))
    return got, want


# ---- packings ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.PACKINGS))
def test_align_equals_the_restatement_at_every_packing(name):
    models, units, stream = cases.packing(name)
    for ls in (0.0, -3.0):
        got, want = _both(models, [stream], [units], ls=ls)
        _assert_equal(got, want, (name, ls))
    assert got["status"].tolist() == [0] and (got["begin"] >= 0).all()
    assert hmm.align_last_kernel_ms() > 0.0


def test_the_looped_body_gives_the_resident_bodys_bits(monkeypatch):
    models, units, stream = cases.packing("5x13")
    opt = np.zeros(len(units), np.uint8)
    opt[[0, 4, 12]] = 1
    one, want = _both(models, [stream, stream[:30]], [units, units], [opt, opt], ls=-1.0)
    _assert_equal(one, want)
    monkeypatch.setenv("ECOZ2_HMM_ALIGN_BODY", "looped")
    _assert_equal(_both(models, [stream, stream[:30]], [units, units], [opt, opt], ls=-1.0)[0], one, "looped")
    monkeypatch.setenv("ECOZ2_HMM_ALIGN_BODY", "resident")
    _assert_equal(_both(models, [stream, stream[:30]], [units, units], [opt, opt], ls=-1.0)[0], one, "resident")


# ---- lengths around the 64-symbol hand-out and around T = L ----------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 4, 63, 64, 65, 129])
def test_lengths_at_three_units(T):
    models = cases.small_models()
    rng = np.random.default_rng(T)
    stream = rng.integers(0, M, T).astype(np.uint16)
    got, want = _both(models, [stream], [np.array([0, 1, 2])], ls=-0.5)
    _assert_equal(got, want, T)
    assert got["status"].tolist() == [1 if T < 3 else 0]  # T = L - 1 (and below): no path; T = L: every unit one frame
    if T == 3:
        assert got["unit"].tolist() == [0, 1, 2] and got["entered"].tolist() == [1, 1, 1]
    if T < 3:
        assert got["log_prob"].tolist() == [NINF]


def test_one_frame_and_one_unit():
    models = cases.small_models()
    got, want = _both(models, [np.array([3], np.uint16)], [np.array([1])])
    _assert_equal(got, want)
    assert got["unit"].tolist() == [0] and got["entered"].tolist() == [1] and got["begin"].tolist() == [0] and got["end"].tolist() == [1]


@pytest.mark.parametrize("body", ["resident", "looped"])
def test_as_many_frames_as_units_forces_the_path(body, monkeypatch):
    monkeypatch.setenv("ECOZ2_HMM_ALIGN_BODY", body)
    e.hmm.set_random_seed(4)
    models = [hmm.init_model(N, M, 0) for N in (5, 3, 4)]  # (random rows without zeros: the forced path has a score)
    units = np.array([0, 1, 2, 2, 1, 0] * 5)
    rng = np.random.default_rng(2)
    stream = rng.integers(0, M, len(units)).astype(np.uint16)
    got, want = _both(models, [stream, stream[:-1]], [units, units], ls=-0.25)
    _assert_equal(got, want, body)
    assert got["status"].tolist() == [0, 1] and got["unit"][:len(units)].tolist() == list(range(len(units)))
    assert np.isfinite(got["log_prob"][0]) and got["log_prob"][1] == NINF


# ---- optional units ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ls", [0.0, -3.0])
def test_a_filler_between_all_units_and_at_both_ends(ls):
    models = cases.planted_models()
    streams, transcripts, optionals = [], [], []
    for fill in ("all", "none", "some"):
        sym, units, opt, _truth = cases.planted(fill)
        streams.append(sym), transcripts.append(units), optionals.append(opt)
    got, want = _both(models, streams, transcripts, optionals, ls)
    _assert_equal(got, want, ls)
    n = len(transcripts[0])
    visited = (got["begin"] >= 0).reshape(3, n)
    filler = optionals[0] != 0
    assert filler[0] and filler[-1]  # (the first and the last unit are optional)
    assert visited[0].all()  # with a filler run everywhere, passing over one never wins
    if ls == -3.0:
        assert not visited[1][filler].any() and visited[1][~filler].all()  # without any, passing over wins everywhere
    assert visited[:, ~filler].all()


def test_a_skip_that_ties_is_not_taken_and_exits_leave_from_the_lowest_state():
    stream, units, opt = cases.skip_tie()
    got, want = _both(cases.skip_tie_models(), [stream], [units], [opt], ls=0.0)
    _assert_equal(got, want)
    assert got["unit"].tolist() == [0, 1, 2] and got["state"].tolist() == [0, 0, 0]
    # uniform models, a class repeated: every comparison ties
    uni = [cases.uniform_model(5), cases.uniform_model(3)]
    rng = np.random.default_rng(3)
    streams = [rng.integers(0, M, n).astype(np.uint16) for n in (7, 70)]
    tr = np.array([0, 0, 1, 0, 1, 1])
    op = np.array([0, 1, 0, 1, 0, 1], np.uint8)
    got, want = _both(uni, streams, [tr, tr], [op, op], ls=0.0)
    _assert_equal(got, want)
    at = np.flatnonzero(got["entered"])
    at = at[(at != 0) & (at != 7)]
    assert len(at) and (got["state"][at - 1] == 0).all()


# ---- L = 1 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mtype", [0, 3])
def test_one_unit_is_hmm_viterbi(mtype):
    e.hmm.set_random_seed(9)
    model = hmm.init_model(7, M, mtype)
    rng = np.random.default_rng(5)
    seqs = [rng.integers(0, M, n).astype(np.uint16) for n in (1, 64, 200)]
    ref = hmm.viterbi(*model, seqs)
    got, want = _both([model], seqs, [np.array([0])] * 3, ls=-2.0)
    _assert_equal(got, want, mtype)
    assert np.array_equal(got["state"], np.concatenate(ref["path"]))
    assert np.array_equal(_bits(got["log_prob"]), _bits(ref["log_prob"])) and np.array_equal(got["status"], ref["status"])
    sym, offs = hmm._pack(seqs)
    assert np.array_equal(_bits(got["score"][offs[1:] - 1]), _bits(ref["log_prob"]))
    assert (got["unit"] == 0).all() and got["begin"].tolist() == [0, 0, 0] and got["end"].tolist() == [1, 64, 200]


# ---- a batch ---------------------------------------------------------------------------------------------------------------------
def _batch():
    models = cases.small_models(seed=11, Ns=(5, 64, 7, 33))
    rng = np.random.default_rng(12)
    streams = [rng.integers(0, M, n).astype(np.uint16) for n in (90, 40, 130)]
    transcripts = [np.array([0, 2, 2, 3]), np.array([1, 0, 3, 1, 2, 0, 0, 2, 2, 1, 3, 3, 1, 1, 0, 2, 1, 1, 3, 1]), np.array([2])]
    optionals = [np.array([1, 0, 1, 0], np.uint8), np.zeros(20, np.uint8), np.zeros(1, np.uint8)]
    return models, streams, transcripts, optionals


def test_a_batch_in_one_launch_and_in_a_launch_per_stream(monkeypatch):
    models, streams, transcripts, optionals = _batch()  # (the second stream takes 17 slots: a launch of its own body)
    one, want = _both(models, streams, transcripts, optionals, ls=-1.0)
    _assert_equal(one, want)
    monkeypatch.setenv("ECOZ2_HMM_ALIGN_TABLE_BYTES", str(40 * (sum(len(models[k][0]) for k in transcripts[1]) + 20)))
    _assert_equal(_both(models, streams, transcripts, optionals, ls=-1.0)[0], one, "a launch per stream")
    monkeypatch.setenv("ECOZ2_HMM_ALIGN_BODY", "looped")
    monkeypatch.delenv("ECOZ2_HMM_ALIGN_TABLE_BYTES")
    _assert_equal(_both(models, streams, transcripts, optionals, ls=-1.0)[0], one, "all looped, one launch")


def test_a_symbol_outside_the_alphabet_is_status_2_and_the_other_streams_are_unaffected():
    models, streams, transcripts, optionals = _batch()
    clean, _want = _both(models, streams, transcripts, optionals, ls=-1.0)
    bad = [s.copy() for s in streams]
    bad[0][70] = M
    got, want = _both(models, bad, transcripts, optionals, ls=-1.0)
    _assert_equal(got, want)
    assert got["status"].tolist() == [2, 0, 0] and got["log_prob"][0] == NINF
    assert got["unit"][:90].tolist() == [0xFFFF] * 90 and got["state"][:90].tolist() == [0xFFFF] * 90 and not got["entered"][:90].any()
    assert got["score"][:90].tolist() == [0.0] + [NINF] * 89 and got["begin"][:4].tolist() == [-1] * 4 and got["end"][:4].tolist() == [-1] * 4
    for key in ("unit", "state", "entered", "score"):
        assert np.array_equal(_bits(got[key][90:]), _bits(clean[key][90:]))
    assert np.array_equal(got["begin"][4:], clean["begin"][4:]) and np.array_equal(_bits(got["log_prob"][1:]), _bits(clean["log_prob"][1:]))


_TORCH_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
torch.cuda.init()  # (torch first: it has to find the device before the library opens it)
from ecoz2rs_amd import hmm
d = np.load(sys.argv[2])
models = list(zip(d["pi"], d["A"], d["B"]))
dev = torch.from_numpy(d["sym"].view(np.int16)).to("cuda:0")
torch.cuda.synchronize()
got = hmm.align(models, dev, d["offs"], d["units"], d["unit_offs"], d["opt"], -1.0)
got.pop("units")
np.savez(sys.argv[3], **got)
print("ok")
"""


def test_symbols_in_a_device_tensor(tmp_path):
    models = cases.small_models(seed=5, Ns=(5, 5, 5))
    rng = np.random.default_rng(9)
    sym, offs = hmm._pack([rng.integers(0, M, n).astype(np.uint16) for n in (200, 0, 90)])
    units, unit_offs, opt = np.array([0, 1, 2, 1, 2, 2, 0], np.int32), np.array([0, 3, 4, 7]), np.array([0, 1, 0, 0, 1, 0, 0], np.uint8)
    ref = hmm.align(models, sym, offs, units, unit_offs, opt, -1.0)
    _assert_equal(ref, R.align(models, sym, offs, units, unit_offs, opt, -1.0))
    assert ref["status"].tolist() == [0, 0, 0] and ref["log_prob"][1] == 0.0 and ref["begin"][3] == -1  # (the empty stream)
    np.savez(tmp_path / "in.npz", pi=np.stack([m[0] for m in models]), A=np.stack([m[1] for m in models]),
             B=np.stack([m[2] for m in models]), sym=sym, offs=offs, units=units, unit_offs=unit_offs, opt=opt)
    r = subprocess.run([sys.executable, "-c", _TORCH_SCRIPT, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
    _assert_equal(np.load(tmp_path / "out.npz"), ref)


# ---- files and the CLI -------------------------------------------------------------------------------------------------------------
def _csv_of(names, units, res, ls, W_ms, O_ms):
    """the CSV of one aligned stream, formatted from the restatement's result"""
    g = lambda v: "%.17g" % v
    doc = "unit,class,begin_frame,end_frame,begin_s,end_s,score\n"
    for l, k, b, en, sc in R.units_of(units, res["begin"], res["end"], res["score"], ls):
        doc += f"{l},{names[k]},{b},{en},{g(b * O_ms / 1000.0)},{g(((en - 1) * O_ms + W_ms) / 1000.0)},{g(sc)}\n"
    return doc.encode()


def test_align_files_and_the_cli_write_the_restatements_csv(tmp_path):
    env = dict(os.environ)
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_GPUS", "ECOZ2_HMM_ALIGN_BODY", "ECOZ2_HMM_ALIGN_TABLE_BYTES"):
        env.pop(k, None)
    W_ms, O_ms, ls = 45, 15, -2.0
    names = ["a", "b", "bg", "c"]  # (the order in which a directory of models is resolved; the cases' classes 0, 1, filler, 2)
    pm = cases.planted_models()
    models = [pm[0], pm[1], pm[3], pm[2]]
    to_file = {0: 0, 1: 1, 2: 3, 3: 2}  # the cases' class index -> the index among the files
    for c, m in zip(names, models):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)
    sym, units_f, _opt, truth = cases.planted("some")
    e.formats.write_seq(str(tmp_path / "x.seq"), "_", M, sym)
    labels = [names[to_file[k]] for k in cases.PLANTED_ORDER]
    # a segment CSV (rows in order) and a selection table (rows out of order, times from the planted boundaries)
    (tmp_path / "x.csv").write_text("segment,class\n" + "".join(f"{i},{c}\n" for i, c in enumerate(labels)))
    rows = [f"{i + 1}\t{truth[2 * i + 1][0] * 0.015}\t{truth[2 * i + 1][1] * 0.015}\t{c}\n" for i, c in enumerate(labels)]
    (tmp_path / "x.txt").write_text("# by hand\nSelection\tBegin Time (s)\tEnd Time (s)\tType\n" + "".join(rows[::-1]))

    def run(*args):
        r = subprocess.run([EXE, *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout, r.stderr)
        return r.stdout

    lms = [R.log_model(*m) for m in models]
    plain = np.array([to_file[k] for k in cases.PLANTED_ORDER], np.int32)
    filled = np.array([to_file[int(k)] for k in units_f], np.int32)
    want_plain = _csv_of(names, plain, R.align_logs(lms, sym, plain, None, ls), ls, W_ms, O_ms)
    res_filled = R.align_logs(lms, sym, filled, _opt, ls)
    want_filled = _csv_of(names, filled, res_filled, ls, W_ms, O_ms)
    assert want_plain != want_filled and (res_filled["begin"] < 0).any()
    common = ["hmm", "align", "--models", "hmms", "--switch-penalty", str(ls), "--sequences", "x.seq"]
    out = run(*common, "--labels", "x.csv", "-c", "plain/x.csv")
    assert (tmp_path / "plain" / "x.csv").read_bytes() == want_plain and "plain/x.csv saved" in out
    run(*common, "--labels", "x.txt", "--filler", "bg", "-c", "filled")
    assert (tmp_path / "filled" / "x.csv").read_bytes() == want_filled
    files = [str(tmp_path / "hmms" / f"{c}.hmm") for c in names]
    hmm.align_files(files, [str(tmp_path / "x.seq")], [str(tmp_path / "x.txt")], ls, filler="bg", csv=tmp_path / "py")
    assert (tmp_path / "py" / "x.csv").read_bytes() == want_filled
    # a .prd through the codebook: the symbols are what `vq quantize` gives, the transcript the same
    rng = np.random.default_rng(3)
    e.formats.write_cbook(str(tmp_path / "m8.cbook"), "_", np.hstack([np.zeros((M, 1)), rng.uniform(-0.8, 0.8, (M, 4))]))
    os.makedirs(tmp_path / "data" / "predictors" / "rec")
    e.formats.write_prd(str(tmp_path / "data" / "predictors" / "rec" / "y.prd"), "rec", rng.uniform(0.1, 1.0, (120, 5)))
    run("vq", "quantize", "--codebook", "m8.cbook", "--predictors", "data/predictors/rec/y.prd")
    _cls, m, ysym = e.formats.read_seq(str(tmp_path / "data" / "sequences" / f"M{M}" / "rec" / "y.seq"))
    assert m == M and len(ysym) == 120
    ysym = np.asarray(ysym, dtype=np.uint16)
    want_y = _csv_of(names, filled, R.align_logs(lms, ysym, filled, _opt, ls), ls, W_ms, O_ms)
    run("hmm", "align", "--models", "hmms", "--switch-penalty", str(ls), "--codebook", "m8.cbook", "--predictors", "data/predictors/rec/y.prd", "--labels",
        "x.csv", "--filler", "bg", "-c", "prd.csv")
    assert (tmp_path / "prd.csv").read_bytes() == want_y
    hmm.align_files(files, [str(tmp_path / "data" / "predictors" / "rec" / "y.prd")], [str(tmp_path / "x.csv")], ls, filler="bg", codebook=tmp_path / "m8.cbook",
                    csv=tmp_path / "py2")
    assert (tmp_path / "py2" / "y.csv").read_bytes() == want_y
