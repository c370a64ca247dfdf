"""`hmm align --posteriors` on the GPU: every output of e2vq_hmm_align_posteriors -- occ, post_path, w0, w1,
w2, the host moments, the raw bits of ln P and the status -- against the numpy restatement
(tests/hmm_align_posterior_restatement.py), bit for bit, at the smallest shape that reaches each code path of
k_hmm_align_posteriors: packed and one-unit slots, 16 slots; the lengths around the 64-frame hand-out and T = L; optional units;
one class in every slot; the shape rows where classes and units part (A in global memory by itself); both forced routes of A; a
batch in one launch and in a launch per stream; the status events; the E-step on the same device; the path of `hmm.align`; the
file form, the CLI and a device tensor."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_align_cases as cases
from . import hmm_align_posterior_restatement as PR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
NINF = float("-inf")
M = cases.M
ENV = ("ECOZ2_HMM_EMBED_A", "ECOZ2_HMM_EMBED_AN", "ECOZ2_HMM_EMBED_CHUNK_BYTES", "ECOZ2_HMM_ALIGN_BODY", "ECOZ2_HMM_ALIGN_TABLE_BYTES")
FIELDS = ("post_path", "w0", "w1", "w2", "present", "begin_mean", "begin_sd", "log_prob")


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _assert_equal(got, want, note=None):
    assert np.array_equal(got["status"], want["status"]), (note, got["status"], want["status"])
    for k in FIELDS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (note, k, a.shape, b.shape)
        bad = np.flatnonzero(_bits(a) != _bits(b))
        assert not len(bad), (note, k, bad[:8], a[bad[:4]], b[bad[:4]])
    if "occ" in got and "occ" in want:
        assert len(got["occ"]) == len(want["occ"])
        for s, (a, b) in enumerate(zip(got["occ"], want["occ"])):
            assert a.shape == b.shape, (note, s, a.shape, b.shape)
            bad = np.argwhere(_bits(a) != _bits(b))
            assert not len(bad), (note, "occ of stream", s, bad[:4])


def _pack(streams, transcripts, optionals=None):
    sym = np.concatenate([np.asarray(s, dtype=np.uint16) for s in streams]) if streams else np.zeros(0, np.uint16)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    units = np.concatenate([np.asarray(u, dtype=np.int32) for u in transcripts]).astype(np.int32)
    unit_offs = np.concatenate([[0], np.cumsum([len(u) for u in transcripts])]).astype(np.int64)
    opt = None if optionals is None else np.concatenate([np.asarray(o, dtype=np.uint8) for o in optionals]).astype(np.uint8)
    return sym, offs, units, unit_offs, opt


def _path_and_ref(args, rng):
    """a per-frame unit and a per-unit reference frame that no decoder made: every value the contract admits, 0xFFFF and a unit
    >= L among them"""
    sym, offs, units, unit_offs, _opt = args
    path, ref = np.zeros(len(sym), np.uint16), np.zeros(len(units), np.int64)
    for s in range(len(offs) - 1):
        T, L = int(offs[s + 1] - offs[s]), int(unit_offs[s + 1] - unit_offs[s])
        p = rng.integers(0, L, T)
        p[rng.uniform(size=T) < 0.1] = 0xFFFF
        p[rng.uniform(size=T) < 0.1] = L
        path[offs[s]:offs[s + 1]] = p
        if T > 0:
            ref[unit_offs[s]:unit_offs[s + 1]] = rng.integers(0, T, L)
    return path, ref


def _both(models, streams, transcripts, optionals=None, ls=0.0, seed=1):
    args = _pack(streams, transcripts, optionals)
    path, ref = _path_and_ref(args, np.random.default_rng(seed))
    return (hmm.align_posteriors(models, *args, ls, path_unit=path, ref=ref), PR.posteriors(models, *args, ls, path_unit=path, ref=ref))


# ---- packings and lengths ------------------------------------------------------------------------------------------------------------
def _optional_every_third(L):
    opt = np.zeros(L, np.uint8)
    opt[::3] = 1
    return opt


@pytest.mark.parametrize("name", ["5x13", "mixed", "64x16"])
def test_every_output_equals_the_restatement_at_every_packing_and_length(name):
    """one launch of the lengths around the 64-frame hand-out and T = L, without and with optional units (the first, the last
    where L - 1 is a multiple of 3, and every third between)"""
    models, units, stream = cases.packing(name)
    L = len(units)
    lengths = sorted({1, 2, 63, 64, 65, 129, L})
    for opt in (None, _optional_every_third(L)):
        streams = [stream[:T] for T in lengths]
        got, want = _both(models, streams, [units] * len(lengths), None if opt is None else [opt] * len(lengths), ls=-0.5)
        _assert_equal(got, want, (name, opt is not None))
        mandatory = L if opt is None else int((opt == 0).sum())
        assert all(st == 1 for st, T in zip(got["status"], lengths) if T < mandatory) and got["status"][-1] == 0
    assert hmm.align_posteriors_last_kernel_ms() > 0.0


def test_one_class_in_every_slot():
    models = cases.small_models(seed=7, Ns=(5, 3), zeros=0.0)
    rng = np.random.default_rng(8)
    stream = rng.integers(0, M, 129).astype(np.uint16)
    units = np.zeros(30, np.int32)  # 12 units of 5 states a slot: three waves
    assert PR.slots_of(models, units) == 3
    opt = np.zeros(30, np.uint8)
    opt[[0, 11, 13, 24, 29]] = 1  # (a path may pass over the last unit of a slot, and over the second of the next)
    for o in (None, opt):
        got, want = _both(models, [stream], [units], None if o is None else [o], ls=-0.25)
        _assert_equal(got, want)
        assert got["status"].tolist() == [0]
        assert np.abs(got["occ"][0].sum(axis=1) - 1.0).max() < 1e-12
        assert (np.abs(got["present"][(o if o is not None else np.zeros(30)) == 0] - 1.0) < 1e-12).all()


def test_seventeen_slots_are_refused_with_the_slot_count():
    models, units, stream = cases.packing("64x17")
    with pytest.raises(Exception, match=r"stream 0: the units take 17 wave-slots of 64 lanes \(at most 16: the alignment posteriors"):
        hmm.align_posteriors(models, stream, [0, len(stream)], units, [0, len(units)])


# ---- the shape rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in cases.SHAPES if n != "64x6c_17u"])
def test_the_shape_rows_where_classes_and_units_part(name):
    models, units, opt, stream = cases.shape(name)
    for ls in (0.0, -3.0):
        got, want = _both(models, [stream], [units], None if opt is None else [opt], ls=ls)
        _assert_equal(got, want, (name, ls))
        assert got["status"].tolist() == [0]


def test_both_forced_routes_of_a_give_the_same_bits(monkeypatch):
    models, streams, transcripts, optionals = cases.unlike_streams()
    base, want = _both(models, streams, transcripts, optionals, ls=-1.0)
    _assert_equal(base, want)
    for a in ("lds", "global"):
        monkeypatch.setenv("ECOZ2_HMM_EMBED_A", a)
        _assert_equal(_both(models, streams, transcripts, optionals, ls=-1.0)[0], base, a)
    monkeypatch.setenv("ECOZ2_HMM_EMBED_A", "shared")
    with pytest.raises(Exception, match="ECOZ2_HMM_EMBED_A=shared: lds or global"):
        _both(models, streams, transcripts, optionals, ls=-1.0)


# ---- batching ------------------------------------------------------------------------------------------------------------------------
def test_a_batch_in_one_launch_and_in_a_launch_per_stream(monkeypatch):
    batches = [cases.unlike_streams(), cases.random_batch(5, 20, max_slots=16, S=12)]
    ones = []
    for models, streams, transcripts, optionals in batches:
        one, want = _both(models, streams, transcripts, optionals, ls=-1.0)
        _assert_equal(one, want)
        ones.append(one)
    monkeypatch.setenv("ECOZ2_HMM_EMBED_CHUNK_BYTES", "1")
    for (models, streams, transcripts, optionals), one in zip(batches, ones):
        args = _pack(streams, transcripts, optionals)
        path, ref = _path_and_ref(args, np.random.default_rng(1))
        _assert_equal(hmm.align_posteriors(models, *args, -1.0, path_unit=path, ref=ref), one, "a launch per stream")


def test_the_status_events_and_a_clean_stream_among_them():
    streams, transcripts, optionals, kinds = cases.event_batch()
    models = cases.event_models()
    got, want = _both(models, streams, transcripts, optionals, ls=-1.0)
    _assert_equal(got, want)
    code = {"clean": 0, "M": 2, "dead": 1, "dead_M": 1, "M_dead": 2}
    assert got["status"].tolist() == [code[k] for k in kinds]
    T, L = cases.EVENT_T, 4
    for s, k in enumerate(kinds):
        if k != "clean":  # every entry of the stream is 0.0, ln P is -inf
            assert not got["occ"][s].any() and not got["post_path"][s * T:(s + 1) * T].any() and got["log_prob"][s] == NINF
            assert not any(got[w][s * L:(s + 1) * L].any() for w in ("w0", "w1", "w2"))
            assert np.isnan(got["begin_mean"][s * L:(s + 1) * L]).all()
    # the clean stream alone: its neighbours change none of its bits
    args = _pack(streams[:1], transcripts[:1], optionals[:1])
    path, ref = _path_and_ref(_pack(streams, transcripts, optionals), np.random.default_rng(1))
    alone = hmm.align_posteriors(models, *args, -1.0, path_unit=path[:T], ref=ref[:L])
    for k in FIELDS:
        n = 1 if k == "log_prob" else T if k == "post_path" else L
        assert np.array_equal(_bits(alone[k]), _bits(got[k][:n])), k
    assert np.array_equal(_bits(alone["occ"][0]), _bits(got["occ"][0]))


# ---- against the E-step and the alignment on the same device -------------------------------------------------------------------------
def test_log_prob_and_status_are_the_embedded_esteps_bits():
    for models, streams, transcripts, optionals in (cases.unlike_streams(), (cases.event_models(),) + cases.event_batch()[:3]):
        args = _pack(streams, transcripts, optionals)
        a = hmm.align_posteriors(models, *args, -1.0, occupancy=False)
        b = hmm.embedded_estep(models, *args, -1.0)
        assert "occ" not in a and np.array_equal(a["status"], b["status"]) and np.array_equal(_bits(a["log_prob"]), _bits(b["log_prob"]))


def test_the_path_of_hmm_align_reads_its_own_column_of_the_occupancy():
    models, streams, transcripts, optionals = cases.unlike_streams()
    args = _pack(streams, transcripts, optionals)
    sym, offs, units, unit_offs, opt = args
    al = hmm.align(models, *args, -1.0)
    assert al["status"].tolist() == [0, 0, 0, 0]
    ref = np.where(al["begin"] < 0, 0, al["begin"])
    got = hmm.align_posteriors(models, *args, -1.0, path_unit=al["unit"], ref=ref)
    _assert_equal(got, PR.posteriors(models, *args, -1.0, path_unit=al["unit"], ref=ref))
    for s in range(4):
        a, b = int(offs[s]), int(offs[s + 1])
        want = got["occ"][s][np.arange(b - a), al["unit"][a:b]]
        assert np.array_equal(_bits(got["post_path"][a:b]), _bits(want)) and (want > 0).all()
    without = hmm.align_posteriors(models, *args, -1.0)
    assert not without["post_path"].any() and np.array_equal(_bits(without["w0"]), _bits(got["w0"]))


# ---- files, the CLI, a device tensor -------------------------------------------------------------------------------------------------
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
got = hmm.align_posteriors(models, dev, d["offs"], d["units"], d["unit_offs"], d["opt"], -1.0, path_unit=d["path"], ref=d["ref"])
occ = got.pop("occ")
np.savez(sys.argv[3], **got, **{f"occ{s}": a for s, a in enumerate(occ)})
print("ok")
"""


def test_symbols_in_a_device_tensor(tmp_path):
    models = cases.small_models(seed=5, Ns=(5, 5, 5))
    rng = np.random.default_rng(9)
    streams = [rng.integers(0, M, n).astype(np.uint16) for n in (100, 0, 70)]
    args = _pack(streams, [np.array([0, 1, 2]), np.array([1]), np.array([2, 2, 0])], [np.array([0, 1, 0]), np.array([0]), np.array([1, 0, 0])])
    path, ref = _path_and_ref(args, np.random.default_rng(2))
    sym, offs, units, unit_offs, opt = args
    base = hmm.align_posteriors(models, *args, -1.0, path_unit=path, ref=ref)
    _assert_equal(base, PR.posteriors(models, *args, -1.0, path_unit=path, ref=ref))
    assert base["status"].tolist() == [0, 1, 0] and base["occ"][1].shape == (0, 1)  # (the empty stream gives nothing)
    np.savez(tmp_path / "in.npz", pi=np.stack([m[0] for m in models]), A=np.stack([m[1] for m in models]),
             B=np.stack([m[2] for m in models]), sym=sym, offs=offs, units=units, unit_offs=unit_offs, opt=opt, path=path, ref=ref)
    r = subprocess.run([sys.executable, "-c", _TORCH_SCRIPT, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
    out = np.load(tmp_path / "out.npz")
    got = {k: out[k] for k in FIELDS + ("status",)}
    got["occ"] = [out[f"occ{s}"] for s in range(3)]
    _assert_equal(got, base)


def test_the_file_form_and_the_cli_report_what_the_array_form_computes(tmp_path):
    env = dict(os.environ)
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_GPUS", "ECOZ2_VQ_QUIET") + ENV:
        env.pop(k, None)
    ls = -1.0
    names = ["a", "b", "bg", "c"]  # (the order in which a directory of models is resolved; the cases' classes 0, 1, filler, 2)
    to_file = {0: 0, 1: 1, 2: 3, 3: 2}
    pm = cases.planted_models()
    models = [pm[0], pm[1], pm[3], pm[2]]
    for c, m in zip(names, models):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)
    stream, units, opt, _truth = cases.planted("some")
    units = np.array([to_file[int(k)] for k in units], np.int32)
    labels = [names[to_file[k]] for k in cases.PLANTED_ORDER]
    e.formats.write_seq(str(tmp_path / "x.seq"), "_", M, stream)
    (tmp_path / "x.csv").write_text("segment,class\n" + "".join(f"{n},{c}\n" for n, c in enumerate(labels)))
    T, L = len(stream), len(units)
    common = ["hmm", "align", "--models", "hmms", "--labels", "x.csv", "--filler", "bg", "--switch-penalty", str(ls)]
    run = lambda *a: subprocess.run([EXE, *common, *a, "--sequences", "x.seq"], cwd=tmp_path, env=env, capture_output=True, text=True,
                                    timeout=600)
    plain = run("-c", "plain.csv")
    r = run("-c", "post.csv", "--posteriors", "--frame-posteriors", "frames")
    assert plain.returncode == 0 and r.returncode == 0, (plain.stdout, r.stdout, r.stderr)
    # the restatement of what the file form computes: the alignment's path and begin, then the posteriors
    args = (stream, np.array([0, T]), units, np.array([0, L]), opt)
    al = hmm.align(models, *args, ls)
    ref = np.where(al["begin"] < 0, 0, al["begin"])
    want = PR.posteriors(models, *args, ls, path_unit=al["unit"], ref=ref)
    assert (al["begin"] < 0).any()  # (a filler the path passes over: it stays out of the CSV)
    rows_plain = (tmp_path / "plain.csv").read_text().splitlines()
    rows = (tmp_path / "post.csv").read_text().splitlines()
    assert [",".join(x.split(",")[:7]) for x in rows] == rows_plain
    assert rows[0].split(",")[7:] == ["posterior", "min_posterior", "p_present", "begin_mean_frame", "begin_sd_frames"]
    visited = [l for l in range(L) if al["begin"][l] >= 0]
    assert len(rows) == 1 + len(visited)
    for row, l in zip(rows[1:], visited):
        b, en = int(al["begin"][l]), int(al["end"][l])
        total = 0.0
        for v in want["post_path"][b:en]:
            total = total + float(v)
        tail = [total / float(en - b), float(want["post_path"][b:en].min()), want["present"][l], want["begin_mean"][l], want["begin_sd"][l]]
        assert row.split(",")[7:] == ["%.17g" % v for v in tail], (l, row)
    frames = (tmp_path / "frames" / "x.csv").read_text().splitlines()
    assert frames[0] == "frame,begin_s,unit,class,posterior" and len(frames) == 1 + T
    assert [x.split(",")[2:] for x in frames[1:]] == [[str(int(al["unit"][t])), names[units[al["unit"][t]]], "%.17g" % want["post_path"][t]]
                                                      for t in range(T)]
    # stdout: the block of the run without the flag, each unit line with its p=, a passed-over unit with its p_present
    lines, lines_plain = r.stdout.splitlines(), plain.stdout.splitlines()
    unit_lines = [x for x in lines if " p=" in x]
    assert len(unit_lines) == len(visited) and [x.rsplit(" p=", 1)[0] for x in unit_lines] == [x for x in lines_plain if x.startswith("    ")]
    passed = [x for x in lines if "(passed over)" in x]
    assert len(passed) == L - len(visited) and all("p_present=" in x for x in passed)
    # the Python file form writes the same bytes
    files = [str(tmp_path / "hmms" / f"{c}.hmm") for c in names]
    hmm.align_files(files, [str(tmp_path / "x.seq")], [str(tmp_path / "x.csv")], ls, filler="bg", csv=tmp_path / "py.csv", posteriors=True,
                    frame_posteriors=tmp_path / "pyframes")
    assert (tmp_path / "py.csv").read_text() == (tmp_path / "post.csv").read_text()
    assert (tmp_path / "pyframes" / "x.csv").read_text() == (tmp_path / "frames" / "x.csv").read_text()
