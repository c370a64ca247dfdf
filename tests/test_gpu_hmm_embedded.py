"""`hmm learn --embedded` on the GPU: every limb of every class's accumulator block, the raw bits of ln P and
the status against the numpy restatement (tests/hmm_embedded_restatement.py) at the smallest shape that reaches each code path
of k_hmm_embed_fb -- packed and one-unit slots, 16 slots; the lengths around the 64-symbol hand-out and around T = L; optional
units at both ends and between all units; one class in every slot; a batch in one launch and in a launch per stream; status 2
inside a batch; symbols in a device tensor; both instantiations and both AN routes --, the training loop against the
restatement's on the bits of every parameter, and the file form and the CLI against the array form."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_embedded_cases as cases
from . import hmm_embedded_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
NINF = float("-inf")
M = cases.M
ENV = ("ECOZ2_HMM_EMBED_A", "ECOZ2_HMM_EMBED_AN", "ECOZ2_HMM_EMBED_CHUNK_BYTES")


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _assert_equal(got, want, note=None):
    assert np.array_equal(got["status"], want["status"]), (note, got["status"], want["status"])
    assert np.array_equal(_bits(got["log_prob"]), _bits(want["log_prob"])), (note, got["log_prob"], want["log_prob"])
    assert len(got["acc"]) == len(want["acc"])
    for k, (a, b) in enumerate(zip(got["acc"], want["acc"])):
        assert a.dtype == b.dtype == np.int64 and a.shape == b.shape
        assert np.array_equal(a, b), (note, "class", k, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


def _both(models, streams, transcripts, optionals=None, ls=0.0):
    args = cases.pack(streams, transcripts, optionals)
    return hmm.embedded_estep(models, *args, ls), R.estep(models, *args, ls)


# ---- packings ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["5x13", "mixed", "64x16"])
def test_the_counts_equal_the_restatement_at_every_packing(name):
    models, units, stream = cases.packing(name)
    for ls in (0.0, -3.0):
        got, want = _both(models, [stream], [units], ls=ls)
        _assert_equal(got, want, (name, ls))
        assert got["status"].tolist() == [0] and np.isfinite(got["log_prob"][0])
    assert hmm.embedded_last_kernel_ms() > 0.0


def test_seventeen_slots_are_refused_with_the_slot_count():
    models, units, stream = cases.packing("64x17")
    with pytest.raises(Exception, match=r"stream 0: the units take 17 wave-slots of 64 lanes \(at most 16"):
        _both(models, [stream], [units])


# ---- lengths around the 64-symbol hand-out and around T = L ----------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 4, 63, 64, 65, 129])
def test_lengths_at_three_units(T):
    models = cases.small_models()
    rng = np.random.default_rng(T)
    stream = rng.integers(0, M, T).astype(np.uint16)
    got, want = _both(models, [stream], [np.array([0, 1, 2])], ls=-0.5)
    _assert_equal(got, want, T)
    assert got["status"].tolist() == [1 if T < 3 else 0]
    if T < 3:
        assert got["log_prob"].tolist() == [NINF]
        for k, a in enumerate(got["acc"]):  # nothing but the stream's mark
            assert a[:-2].tolist() == [0] * (len(a) - 2) and a[-2:].tolist() == [0, 1], k


# ---- optional units, repeats -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ls", [0.0, -3.0])
def test_a_filler_between_all_units_and_at_both_ends(ls):
    models = cases.planted_models()
    streams, transcripts, optionals = [], [], []
    for fill in ("all", "none", "some"):
        sym, units, opt, _truth = cases.planted(fill)
        streams.append(sym), transcripts.append(units), optionals.append(opt)
    assert optionals[0][0] and optionals[0][-1]
    got, want = _both(models, streams, transcripts, optionals, ls)
    _assert_equal(got, want, ls)
    assert got["status"].tolist() == [0, 0, 0]
    assert [int(a[-2]) for a in got["acc"]] == [3, 3, 3, 3]


def test_one_class_in_every_slot_adds_to_one_cell():
    models = cases.small_models(seed=7, Ns=(5, 3), zeros=0.0)
    rng = np.random.default_rng(8)
    stream = rng.integers(0, M, 150).astype(np.uint16)
    units = np.zeros(30, np.int32)  # 12 units of 5 states a slot: three waves add to the cells of class 0
    assert R.slots_of(models, units) == 3
    got, want = _both(models, [stream], [units], ls=-0.25)
    _assert_equal(got, want)
    assert got["status"].tolist() == [0] and not got["acc"][1].any()  # (the unnamed class has no count and no mark)


# ---- a batch ---------------------------------------------------------------------------------------------------------------------
def _batch():
    models = cases.small_models(seed=11, Ns=(5, 64, 7, 33))
    rng = np.random.default_rng(12)
    streams = [rng.integers(0, M, n).astype(np.uint16) for n in (90, 40, 130)]
    transcripts = [np.array([0, 2, 2, 3]), np.array([1, 0, 3, 1, 2, 0, 0, 2, 2, 1, 3, 3, 1, 1, 0, 2]), np.array([2])]
    optionals = [np.array([1, 0, 1, 0], np.uint8), np.zeros(16, np.uint8), np.zeros(1, np.uint8)]
    return models, streams, transcripts, optionals


def test_a_batch_in_one_launch_and_in_a_launch_per_stream(monkeypatch):
    models, streams, transcripts, optionals = _batch()
    one, want = _both(models, streams, transcripts, optionals, ls=-1.0)
    _assert_equal(one, want)
    monkeypatch.setenv("ECOZ2_HMM_EMBED_CHUNK_BYTES", "1")
    _assert_equal(_both(models, streams, transcripts, optionals, ls=-1.0)[0], one, "a launch per stream")


def test_a_symbol_outside_the_alphabet_is_status_2_and_the_stream_adds_nothing():
    models, streams, transcripts, optionals = _batch()
    bad = [s.copy() for s in streams]
    bad[0][70] = M
    got, want = _both(models, bad, transcripts, optionals, ls=-1.0)
    _assert_equal(got, want)
    assert got["status"].tolist() == [2, 0, 0] and got["log_prob"][0] == NINF
    without, _w = _both(models, streams[1:], transcripts[1:], optionals[1:], ls=-1.0)
    for k, (a, b) in enumerate(zip(got["acc"], without["acc"])):  # every limb as the batch without it; the mark apart
        assert np.array_equal(a[:-1], b[:-1]) and a[-1] == b[-1] + (1 if k in (0, 2, 3) else 0), k


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
got = hmm.embedded_estep(models, dev, d["offs"], d["units"], d["unit_offs"], d["opt"], -1.0)
np.savez(sys.argv[3], log_prob=got["log_prob"], status=got["status"], **{f"acc{k}": a for k, a in enumerate(got["acc"])})
print("ok")
"""


def test_symbols_in_a_device_tensor(tmp_path):
    models = cases.small_models(seed=5, Ns=(5, 5, 5))
    rng = np.random.default_rng(9)
    sym, offs = hmm._pack([rng.integers(0, M, n).astype(np.uint16) for n in (200, 0, 90)])
    units, unit_offs, opt = np.array([0, 1, 2, 1, 2, 2, 0], np.int32), np.array([0, 3, 4, 7]), np.array([0, 1, 0, 0, 1, 0, 0], np.uint8)
    ref = hmm.embedded_estep(models, sym, offs, units, unit_offs, opt, -1.0)
    _assert_equal(ref, R.estep(models, sym, offs, units, unit_offs, opt, -1.0))
    assert ref["status"].tolist() == [0, 1, 0]  # (the empty stream gives nothing)
    np.savez(tmp_path / "in.npz", pi=np.stack([m[0] for m in models]), A=np.stack([m[1] for m in models]),
             B=np.stack([m[2] for m in models]), sym=sym, offs=offs, units=units, unit_offs=unit_offs, opt=opt)
    r = subprocess.run([sys.executable, "-c", _TORCH_SCRIPT, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
    out = np.load(tmp_path / "out.npz")
    _assert_equal(dict(log_prob=out["log_prob"], status=out["status"], acc=[out[f"acc{k}"] for k in range(3)]), ref)


# ---- the instantiations and the routes ----------------------------------------------------------------------------------------------
def test_both_instantiations_and_both_routes_give_the_same_limbs(monkeypatch):
    models, streams, transcripts, optionals = _batch()
    base, want = _both(models, streams, transcripts, optionals, ls=-1.0)
    _assert_equal(base, want)
    for a in ("lds", "global"):
        for an in ("lds", "global"):
            monkeypatch.setenv("ECOZ2_HMM_EMBED_A", a)
            monkeypatch.setenv("ECOZ2_HMM_EMBED_AN", an)
            _assert_equal(_both(models, streams, transcripts, optionals, ls=-1.0)[0], base, (a, an))
    monkeypatch.setenv("ECOZ2_HMM_EMBED_AN", "shared")
    with pytest.raises(Exception, match="ECOZ2_HMM_EMBED_AN=shared: lds or global"):
        _both(models, streams, transcripts, optionals, ls=-1.0)


# ---- the training loop -------------------------------------------------------------------------------------------------------------
def _planted_training():
    streams, transcripts, optionals = cases.planted_batch(fills=("some", "all"), seeds=(20, 21))
    return cases.blurred(cases.planted_models()), cases.pack(streams, transcripts, optionals)


@pytest.mark.parametrize("epsilon", [0.0, 1e-5])
def test_three_iterations_equal_the_restatements_on_the_bits(epsilon):
    start, args = _planted_training()
    got, hist = hmm.train_embedded(start, *args, -1.0, epsilon, -1e300, 3)
    want, whist = R.train(start, *args, -1.0, epsilon, -1e300, 3)
    assert len(hist) == 3 and np.array_equal(_bits(hist), _bits(np.array(whist)))
    for k, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(("pi", "A", "B"), g, w):
            assert np.array_equal(_bits(a), _bits(b)), (k, name)
    assert hist[2] > hist[0]
    for k in range(3):  # the left-to-right zeros are still exact zeros
        assert (got[k][1][np.tril_indices(3, -1)] == 0.0).all() and got[k][0][1:].tolist() == [0.0, 0.0]
    # the stop on val_auto: the E-step that stops gets no M-step
    got2, hist2 = hmm.train_embedded(start, *args, -1.0, epsilon, 1e300, -1)
    want2, whist2 = R.train(start, *args, -1.0, epsilon, 1e300, -1)
    assert len(hist2) == len(whist2) == 2 and np.array_equal(_bits(hist2), _bits(np.array(whist2)))
    assert all(np.array_equal(_bits(a), _bits(b)) for g, w in zip(got2, want2) for a, b in zip(g, w))


def test_an_unnamed_class_keeps_its_bytes_and_no_usable_stream_is_an_error():
    start, args = _planted_training()
    extra = cases.small_models(seed=2, Ns=(6,))[0]
    got, _hist = hmm.train_embedded(start + [extra], *args, -1.0, 1e-5, -1e300, 2)
    assert all(np.asarray(a).tobytes() == np.asarray(b, dtype=np.float64).tobytes() for a, b in zip(got[4], extra))
    assert not np.array_equal(got[0][2], start[0][2])
    sym, offs, units, unit_offs, opt = args
    with pytest.raises(Exception, match="no stream can be explained by its transcript"):
        hmm.train_embedded(start, sym[:3], np.array([0, 3]), units[:unit_offs[1]], unit_offs[:2], opt[:unit_offs[1]], -1.0)


# ---- files and the CLI -------------------------------------------------------------------------------------------------------------
def test_the_file_form_and_the_cli_train_what_the_array_form_trains(tmp_path, capfd):
    env = dict(os.environ)
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_GPUS", "ECOZ2_VQ_QUIET") + ENV:
        env.pop(k, None)
    ls, eps = -1.0, 1e-5
    names = ["a", "b", "bg", "c"]  # (the order in which a directory of models is resolved; the cases' classes 0, 1, filler, 2)
    to_file = {0: 0, 1: 1, 2: 3, 3: 2}
    bl = cases.blurred(cases.planted_models())
    models = [bl[0], bl[1], bl[3], bl[2]]
    for c, m in zip(names, models):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)
    streams, transcripts, optionals = cases.planted_batch(fills=("some", "all"), seeds=(20,))
    labels = [names[to_file[k]] for k in cases.PLANTED_ORDER]
    seqs, labs = [], []
    for i, s in enumerate(streams):
        e.formats.write_seq(str(tmp_path / f"x{i}.seq"), "_", M, s)
        (tmp_path / f"x{i}.csv").write_text("segment,class\n" + "".join(f"{n},{c}\n" for n, c in enumerate(labels)))
        seqs.append(f"x{i}.seq"), labs.append(f"x{i}.csv")
    filled = [np.array([to_file[int(k)] for k in u], np.int32) for u in transcripts]
    args = cases.pack(streams, filled, optionals)
    want, whist = hmm.train_embedded(models, *args, ls, eps, 0.3, 4)
    r = subprocess.run([EXE, "hmm", "learn", "--embedded", "--models", "hmms", "--labels", *labs, "--filler", "bg", "--switch-penalty", str(ls),
                        "-e", str(eps), "-a", "0.3", "-I", "4", "-o", "out", "--sequences", *seqs], cwd=tmp_path, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.count("  it=") == len(whist) and f"{len(whist)} E-step(s); 4 model(s) saved in out" in r.stdout

    def check(out_dir):
        for c, w in zip(names, want):
            g = hmm.load_model(out_dir / f"{c}.hmm")
            assert all(np.array_equal(_bits(np.asarray(a)), _bits(b)) for a, b in zip(g[-3:], w)), c
        rows = (out_dir / "embedded.csv").read_text().splitlines()
        assert rows[0] == "iteration,sum_log_prob,streams_used,streams_skipped"
        assert rows[1:] == [f"{i},{'%.17g' % L},{len(streams)},0" for i, L in enumerate(whist)]

    check(tmp_path / "out")
    files = [str(tmp_path / "hmms" / f"{c}.hmm") for c in names]
    seen = []
    hmm.learn_embedded_files(files, [str(tmp_path / s) for s in seqs], [str(tmp_path / l) for l in labs], tmp_path / "py", ls, filler="bg",
                             hmm_epsilon=eps, val_auto=0.3, max_iterations=4, callback=lambda v, x: seen.append((v, x)))
    check(tmp_path / "py")
    assert seen == [("sum_log_prob", L) for L in whist]
    # a stream its transcript cannot explain is named on stderr with the iteration, skipped, and counted in the CSV
    e.formats.write_seq(str(tmp_path / "short.seq"), "_", M, streams[0][:3])
    capfd.readouterr()
    hmm.learn_embedded_files(files, [str(tmp_path / s) for s in seqs + ["short.seq"]], [str(tmp_path / l) for l in labs + [labs[0]]],
                             tmp_path / "py3", ls, filler="bg", hmm_epsilon=eps, val_auto=0.3, max_iterations=2)
    err = capfd.readouterr().err
    assert err.count("skipped") == 1 and "short.seq: it=0: skipped: no path of probability > 0 through its transcript" in err
    rows = (tmp_path / "py3" / "embedded.csv").read_text().splitlines()
    assert [r.split(",", 2)[2] for r in rows[1:]] == [f"{len(streams)},1"] * 2
    assert [r.split(",")[1] for r in rows[1:]] == ["%.17g" % L for L in whist[:2]]  # (the other streams' sums are not touched)
    # an output directory that would overwrite an input model
    r = subprocess.run([EXE, "hmm", "learn", "--embedded", "--models", "hmms", "--labels", *labs, "--filler", "bg", "-o", "hmms", "--sequences", *seqs],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "would overwrite an input model" in r.stdout
    assert hmm.load_model(tmp_path / "hmms" / "a.hmm")[-1].tobytes() == np.asarray(models[0][2]).tobytes()
