"""`hmm segment --class-transitions` on the GPU: cls, state, entered, the raw bits of exit_score and
ln P*, and status against the numpy restatement (tests/hmm_segment_trans_restatement.py) under asymmetric random prices
with some -inf, at the smallest shape that reaches each code path of k_hmm_segment_trans -- the 64-symbol hand-out, packed
and one-class slots, 16 slots, each of the four (lA, lt) placements --; the status codes and the empty stream; the same
bits under a small table budget and from symbols already on the device; ties on duplicated classes; the uniform matrix
against `hmm segment`; the refusal of 17 slots; the file form against the array call and, with a uniform file, against the
run without one."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_segment_trans_cases as cases
from . import hmm_segment_trans_restatement as RT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
NINF = float("-inf")
KEYS = ("cls", "state", "entered", "exit_score", "log_prob", "status")
# name: (N of every class, M, stream lengths) -- and where lA and lt live
SHAPES = {
    "1": ([1], 4, (1, 2)),                                    # K = 1: every entry re-enters the one class
    "handout": ([5, 3, 4], 8, (63, 64, 65, 129)),             # the 64-symbol hand-out
    "5x12": ([5] * 12, 8, (70,)),                             # one wave, 4 idle lanes
    "40_40": ([40, 40], 8, (70,)),                            # the second class opens the next slot
    "mixed": ([3, 64, 7, 7, 33], 8, (70,)),                   # packed slots next to one-class slots (v_readlane)
    "64x16": ([64] * 16, 8, (66,)),                           # 16 slots; lA from global memory, lt in LDS
    "1x1024": ([1] * 1024, 4, (8,)),                          # 16 full slots; lA in LDS, lt from global memory
    "40_1x24_x14": (([40] + [1] * 24) * 14, 4, (8,)),         # lA and lt from global memory
}


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _assert_equal(got, want, note=None, keys=KEYS):
    for key in keys:
        a, b = _bits(got[key]), _bits(want[key])
        assert a.dtype == b.dtype and np.array_equal(a, b), (key, note, np.flatnonzero(a != b)[:5] if a.shape == b.shape else (a.shape, b.shape))


def _init_models(Ns, M, mtype=0, seed=5):
    e.hmm.set_random_seed(seed)
    return [hmm.init_model(N, M, mtype) for N in Ns]


def _streams(rng, M, lengths):
    return [rng.integers(0, M, n).astype(np.uint16) for n in lengths]


@pytest.mark.parametrize("name", list(SHAPES))
def test_segment_trans_equals_the_restatement(name):
    Ns, M, lengths = SHAPES[name]
    models = _init_models(Ns, M)
    rng = np.random.default_rng(len(Ns) + M)
    sym, offs = hmm._pack(_streams(rng, M, lengths))
    lt = cases.random_prices(rng, len(Ns))
    got = hmm.segment_trans(models, sym, offs, lt)
    want = RT.segment_trans(models, sym, offs, lt)
    _assert_equal(got, want, name)
    for s, segs in enumerate(got["segments"]):
        a, b = offs[s], offs[s + 1]
        ref = RT.segments_of(want["cls"][a:b], want["entered"][a:b], want["exit_score"][a:b], want["log_prob"][s], lt)
        assert [(g["begin"], g["end"], g["cls"]) for g in segs] == [r[:3] for r in ref]
        assert np.array_equal(_bits(np.array([g["log_prob"] for g in segs])), _bits(np.array([r[3] for r in ref])))
    assert hmm.segment_trans_last_kernel_ms() > 0.0


@pytest.mark.parametrize("mtype", [1, 2, 3])  # uniform (every comparison a tie), cascades (-inf in pi and A)
def test_ties_and_forbidden_moves_inside_the_models(mtype):
    Ns, M = [5, 3, 4, 5], 8
    models = _init_models(Ns, M, mtype)
    rng = np.random.default_rng(mtype)
    sym, offs = hmm._pack(_streams(rng, M, (1, 40, 65)))
    for lt in (cases.random_prices(rng, 4), np.full((4, 4), NINF), np.zeros((4, 4))):
        _assert_equal(hmm.segment_trans(models, sym, offs, lt), RT.segment_trans(models, sym, offs, lt), mtype)


def test_streams_of_every_status_in_one_call():
    e.hmm.set_random_seed(5)
    models = []
    for N in (5, 3, 7):
        pi, A, B = hmm.init_model(N, 8, 3)
        B[:, 5] = 0.0  # symbol 5 cannot be emitted by any state of any class
        models.append((pi, A, B))
    seqs = [np.array([1, 2, 3, 4, 1, 2], dtype=np.uint16), np.zeros(0, dtype=np.uint16), np.array([1, 2, 9, 2, 3], dtype=np.uint16),
            np.array([1, 5, 2, 3], dtype=np.uint16), np.array([3, 2, 1], dtype=np.uint16)]
    sym, offs = hmm._pack(seqs)
    lt = cases.random_prices(np.random.default_rng(1), 3)
    got = hmm.segment_trans(models, sym, offs, lt)
    assert got["status"].tolist() == [0, 0, 2, 1, 0]
    assert got["log_prob"][1] == 0.0 and got["log_prob"][[2, 3]].tolist() == [NINF] * 2 and np.isfinite(got["log_prob"][[0, 4]]).all()
    assert got["cls"][offs[2]:offs[3]].tolist() == [0xFFFF] * 5 and got["state"][offs[2]:offs[3]].tolist() == [0xFFFF] * 5
    assert got["entered"][offs[2]:offs[3]].tolist() == [0] * 5 and got["exit_score"][offs[2]:offs[3]].tolist() == [0.0] + [NINF] * 4
    _assert_equal(got, RT.segment_trans(models, sym, offs, lt))  # status 1 still writes the path, by the same rules


@pytest.mark.parametrize("name", ["5x12", "mixed"])
def test_a_small_table_budget_gives_the_same_bits(name, monkeypatch):
    Ns, M, _lengths = SHAPES[name]
    models = _init_models(Ns, M, seed=77)
    rng = np.random.default_rng(4)
    sym, offs = hmm._pack(_streams(rng, M, rng.integers(0, 60, 12)))
    lt = cases.random_prices(rng, len(Ns))
    one = hmm.segment_trans(models, sym, offs, lt)
    _assert_equal(one, RT.segment_trans(models, sym, offs, lt))
    for budget in ("1", str((2 * sum(Ns) + 12 * len(Ns)) * 100)):  # one stream per launch; a few streams per launch
        monkeypatch.setenv("ECOZ2_HMM_SEGMENT_CHUNK_BYTES", budget)
        _assert_equal(hmm.segment_trans(models, sym, offs, lt), one, budget)


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
got = hmm.segment_trans(models, dev, d["offs"], d["lt"])
got.pop("segments")
np.savez(sys.argv[3], **got)
print("ok")
"""


def test_symbols_in_a_device_tensor(tmp_path):
    models = _init_models([5, 5, 5], 64, seed=3)
    rng = np.random.default_rng(9)
    sym, offs = hmm._pack(_streams(rng, 64, (200, 0, 90)))
    lt = cases.random_prices(rng, 3)
    ref = hmm.segment_trans(models, sym, offs, lt)
    _assert_equal(ref, RT.segment_trans(models, sym, offs, lt))
    np.savez(tmp_path / "in.npz", pi=np.stack([m[0] for m in models]), A=np.stack([m[1] for m in models]),
             B=np.stack([m[2] for m in models]), sym=sym, offs=offs, lt=lt)
    r = subprocess.run([sys.executable, "-c", _TORCH_SCRIPT, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
    _assert_equal(np.load(tmp_path / "out.npz"), ref)


def test_duplicated_classes_tie_to_the_lowest_index():
    base = _init_models([5, 3], 8, seed=12)
    models = [base[0], base[1], base[0], base[1], base[0]]
    dup = [0, 1, 0, 1, 0]
    rng = np.random.default_rng(6)
    small = cases.random_prices(rng, 2, forbidden=0.0) / 20.0  # (cheap enough that the paths do switch)
    lt = small[np.ix_(dup, dup)]  # a copy pays what its original pays: every maximum over the sources is reached twice or more
    sym, offs = hmm._pack(_streams(rng, 8, (1, 2, 64, 90)))
    got = hmm.segment_trans(models, sym, offs, lt)
    _assert_equal(got, RT.segment_trans(models, sym, offs, lt))
    # where a segment could start in any copy of a class, the one a path leaves from is the lowest
    firsts = set(int(o) for o in offs[:-1])
    left = [int(got["cls"][t - 1]) for t in np.flatnonzero(got["entered"]) if int(t) not in firsts]  # (the class of frame t - 1)
    assert left and all(k < 2 for k in left)


@pytest.mark.parametrize("case", [c[0] for c in cases.uniform_cases()])
def test_a_uniform_matrix_is_hmm_segment(case):
    _name, models, streams = next(c for c in cases.uniform_cases() if c[0] == case)
    sym, offs = hmm._pack(streams)
    K = len(models)
    got = hmm.segment_trans(models, sym, offs, np.full((K, K), cases.UNIFORM_PRICE))
    ref = hmm.segment(models, sym, offs, cases.UNIFORM_PRICE)
    _assert_equal(got, ref, case, keys=("cls", "state", "entered", "log_prob", "status"))
    at = np.flatnonzero(ref["entered"])
    assert np.array_equal(_bits(got["exit_score"][at]), _bits(ref["gbest"][at]))


def test_seventeen_slots_are_refused():
    models = _init_models([64] * 17, 4)
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.segment_trans(models, np.zeros(4, np.uint16), [0, 4], np.zeros((17, 17)))
    assert "the classes take 17 wave-slots of 64 lanes (at most 16" in str(ei.value)


# ---- files -----------------------------------------------------------------------------------------------------------------
def test_the_file_form_equals_the_array_call_and_a_uniform_file_changes_nothing(tmp_path, capfd):
    env = dict(os.environ)
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_GPUS", "ECOZ2_HMM_SEGMENT_BODY", "ECOZ2_HMM_SEGMENT_CHUNK_BYTES"):
        env.pop(k, None)
    M, W_ms, O_ms, ls = 16, 45, 15, -2.0
    rng = np.random.default_rng(11)
    names = ["rain", "ship", "whale"]  # (the order in which a directory of models is resolved)
    models = []
    for k, (pi, A, B) in enumerate(_init_models((3, 5, 7), M, seed=21)):  # class k leans to the symbols 5 k .. 5 k + 4
        B[:, 5 * k:5 * k + 5] *= 20.0
        models.append((pi, A, B / B.sum(axis=1, keepdims=True)))
    for c, m in zip(names, models):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)
    sym = np.concatenate([rng.integers(5 * k, 5 * k + 5, 50) for k in (0, 2, 1, 0, 1, 2, 2, 0)]).astype(np.uint16)
    e.formats.write_seq(str(tmp_path / "x.seq"), "_", M, sym)
    file_lt = cases.random_prices(rng, 3)
    order = [2, 0, 1]  # the file names the classes in an order of its own
    hmm.write_class_transitions(tmp_path / "t.csv", [names[k] for k in order], file_lt[np.ix_(order, order)])
    hmm.write_class_transitions(tmp_path / "zero.csv", names, np.zeros((3, 3)))

    def run(*args):
        r = subprocess.run([EXE, *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout, r.stderr)
        return r.stdout

    common = ["hmm", "segment", "--models", "hmms", "--switch-penalty", str(ls), "--sequences", "x.seq"]
    out = run(*common, "-c", "with/x.csv", "--class-transitions", "t.csv")
    want = (tmp_path / "with" / "x.csv").read_bytes()
    lt = file_lt + ls
    got = hmm.segment_trans(models, sym, [0, len(sym)], lt)
    _assert_equal(got, RT.segment_trans(models, sym, [0, len(sym)], lt))
    names_c, _k = hmm._strs(names)
    capfd.readouterr()
    assert e.lib.e2vq_hmm_segment_trans_report(b"x.seq", len(sym), 3, names_c, W_ms, O_ms, got["cls"].ctypes.data,
                                               got["entered"].ctypes.data, got["exit_score"].ctypes.data, float(got["log_prob"][0]),
                                               ls, np.ascontiguousarray(lt).ctypes.data, str(tmp_path / "arr.csv").encode()) == 0
    block = capfd.readouterr().out
    assert (tmp_path / "arr.csv").read_bytes() == want
    rows = want.decode().split("\n")
    assert rows[0] == "segment,begin_frame,end_frame,begin_s,end_s,class,log_prob,log_prob_per_frame" and len(rows) == len(got["segments"][0]) + 2
    assert len(got["segments"][0]) > 1 and rows[-2].split(",")[2] == str(len(sym))
    strip = lambda text: [l for l in text.split("\n") if l and not l.endswith(" saved")]
    assert strip(block) == strip(out)[-len(strip(block)):]
    # the Python mirror of the file call
    hmm.segment_files([str(tmp_path / "hmms" / f"{c}.hmm") for c in names], [str(tmp_path / "x.seq")], ls, csv=tmp_path / "py",
                      class_transitions=tmp_path / "t.csv")
    assert (tmp_path / "py" / "x.csv").read_bytes() == want
    # a file of zeros adds nothing to the switch penalty: the bytes of the run without it
    run(*common, "-c", "plain/x.csv")
    run(*common, "-c", "zero/x.csv", "--class-transitions", "zero.csv")
    assert (tmp_path / "zero" / "x.csv").read_bytes() == (tmp_path / "plain" / "x.csv").read_bytes()
    assert (tmp_path / "plain" / "x.csv").read_bytes() != want
