"""`vq quantize --codebooks` on the GPU: a resident set of codebooks quantized over in one pass must give,
per codebook, the single call's symbols and distortions bit for bit -- on arrays (CodebookSet against VqSession per codebook
and the oracle), at every block shape, pointer alignment and output stride, with ties, on the route the set promises
(launch counts), and on files (e2vq_vq_quantize_codebooks against a loop of ecoz2_vq_quantize calls in ascending M: .seq
trees and stdout), for any ECOZ2_VQ_GPUS and ECOZ2_VQ_QUANTIZE_CHUNK, through the CLI, and into `hmm learn --grid`.

ecoz2_vq_quantize runs the same planner and worker with a set of one codebook, so for M < 256 both sides of the file
comparisons launch k_quantize_set: those tests pin the K-fold bookkeeping (rows of a slot, result records, ascending M, .tmp
handling), not the kernel.  The kernel's independent checks are the array tests here against the CPU oracle and the existing
ecoz2_vq_quantize-against-oracle tests."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import vq
from tests.test_gpu_prefilter import _DeviceBuffer
from tests.vq_classes_common import _bits, _class_frames, _read_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
EPS = 0.05
SET_MS = [1, 2, 3, 16, 17, 100, 256, 1024, 2048]
_ladders = {}


def _ladder(P, max_M=2048):
    """the levels M = 1, 2, 4, .. max_M of one seeded ladder (M = 1: the initial codebook)"""
    if (P, max_M) not in _ladders:
        frames = e.synth.synth_frames_kind(411 + P, 1, 4, 0.05, P, 0, 12000)
        levels = {}
        with e.VqSession(P) as s:
            s.set_frames(frames)
            s.prepare()
            s.init_codebook()
            levels[1] = s.get_codebook()
            M = 2
            while M <= max_M:
                s.learn(EPS, M)
                levels[M] = s.get_codebook()
                M *= 2
        _ladders[(P, max_M)] = levels
    return _ladders[(P, max_M)]


def _set_codebooks(P, Ms=SET_MS):
    """the odd sizes: leading rows of the next level"""
    lv = _ladder(P)
    return [lv[1 << max(M - 1, 0).bit_length()][:M].copy() for M in Ms]


def _frames(P, T, seed=77):
    return e.synth.synth_frames_kind(seed + P, 1, 4, 0.05, P, 5000, T)


def _single(P, cb, frames):
    with e.VqSession(P) as s:
        s.set_codebook(cb)
        return s.quantize(frames)


@pytest.mark.parametrize("P", [12, 36, 40, 48, 100])
def test_set_equals_sessions_and_oracle(oracle, P):
    cbs = _set_codebooks(P)
    frames = _frames(P, 4097 if P != 36 else 6000)
    with e.CodebookSet(P, cbs) as cs:
        sym, dmin = cs.quantize(frames)
        only_sym = cs.quantize(frames, want_dmin=False)
    assert sym.shape == dmin.shape == (len(cbs), len(frames)) and sym.dtype == np.uint16
    assert np.array_equal(only_sym, sym)
    for k, cb in enumerate(cbs):
        s1, d1 = _single(P, cb, frames)
        assert np.array_equal(sym[k], s1), (P, len(cb))
        assert np.array_equal(_bits(dmin[k]), _bits(d1)), (P, len(cb))
        if P == 36 or len(cb) <= 256:
            so, do = oracle.quantize(oracle.reflections_to_cq(cb), frames)
            assert np.array_equal(sym[k], so), (P, len(cb))
            assert np.array_equal(_bits(dmin[k]), _bits(do)), (P, len(cb))


@pytest.mark.parametrize("T", [1, 63, 64, 65, 128, 129, 4097])
def test_block_shapes(T):
    P = 36
    cbs = _set_codebooks(P)
    frames = _frames(P, T, seed=5)
    with e.CodebookSet(P, cbs) as cs:
        sym, dmin = cs.quantize(frames)
    for k, cb in enumerate(cbs):
        s1, d1 = _single(P, cb, frames)
        assert np.array_equal(sym[k], s1) and np.array_equal(_bits(dmin[k]), _bits(d1)), (T, len(cb))


@pytest.mark.parametrize("first,T", [(1, 4097), (3, 65), (1, 1), (2, 300)])
def test_device_pointers_alignment_and_strides(first, T):
    """frames at an odd frame of a larger device buffer (37 doubles per frame: 8-byte aligned only) and at an even one (16-byte
    aligned: the set kernel), output rows longer than T: the gaps keep their pattern (0xFF bytes)"""
    P = 36
    cbs = _set_codebooks(P)
    K = len(cbs)
    host = _frames(P, first + T + 3, seed=9)
    buf = _DeviceBuffer(host.nbytes)
    buf.from_host(host)
    ptr = buf.ptr.value + first * (P + 1) * 8
    assert ptr % 16 == (8 if first % 2 else 0)
    ss, ds = T + 37, T + 5
    sym, dmin = _DeviceBuffer(2 * K * ss), _DeviceBuffer(8 * K * ds)
    with e.CodebookSet(P, cbs) as cs:
        cs.quantize_device(ptr, T, sym.ptr.value, ss, dmin.ptr.value, ds)
        before = cs.launch_counts()
        cs.quantize_device(ptr, T, sym.ptr.value, ss)  # (no distortions wanted)
        cs.set_stream(None)  # (synchronises the set's stream)
        after = cs.launch_counts()
    sym_h = sym.to_host(np.uint16).reshape(K, ss)
    dmin_h = dmin.to_host(np.uint64).reshape(K, ds)
    n_pre = sum(1 for cb in cbs if len(cb) >= 256)
    assert before == ((0, K) if first % 2 else (1, n_pre))
    assert after == tuple(2 * x for x in before)
    for k, cb in enumerate(cbs):
        s1, d1 = _single(P, cb, host[first:first + T])
        assert np.array_equal(sym_h[k, :T], s1) and np.array_equal(dmin_h[k, :T], _bits(d1)), (first, T, len(cb))
    assert (sym_h[:, T:] == 0xFFFF).all() and (dmin_h[:, T:] == 0xFFFFFFFFFFFFFFFF).all()
    for b in (buf, sym, dmin):
        b.free()


_TORCH_SCRIPT = r"""
import sys
import torch
torch.cuda.init()
sys.path.insert(0, sys.argv[1])
import numpy as np
import ecoz2rs_amd as e
P, T, first = 36, 1000, 1
lv = np.load(sys.argv[2])
cbs = [lv[:M].copy() for M in (3, 16, 100, 256)]
host = e.synth.synth_frames_kind(5, 1, 4, 0.05, P, 0, first + T + 1)
buf = torch.from_numpy(host).to("cuda:0")
for off in (first, first + 1):  # 8-byte aligned only, then 16-byte aligned
    view = buf[off:off + T]
    assert view.data_ptr() % 16 == (8 if off % 2 else 0)
    sym = torch.full((len(cbs), T + 9), -2, dtype=torch.int16, device="cuda:0")
    dmin = torch.full((len(cbs), T + 3), -7.25, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    with e.CodebookSet(P, cbs) as cs:
        cs.quantize_device(view, T, sym, T + 9, dmin, T + 3)
        cs.set_stream(None)
        assert cs.launch_counts() == ((0, 4) if off % 2 else (1, 1)), cs.launch_counts()
    sym_h, dmin_h = sym.cpu().numpy().view(np.uint16), dmin.cpu().numpy()
    assert (sym_h[:, T:] == 0xFFFE).all() and (dmin_h[:, T:] == -7.25).all()
    for k, cb in enumerate(cbs):
        with e.VqSession(P) as s:
            s.set_codebook(cb)
            s1, d1 = s.quantize(host[off:off + T])
        assert np.array_equal(sym_h[k, :T], s1) and np.array_equal(dmin_h[k, :T].view(np.uint64), d1.view(np.uint64)), (off, k)
print("torch tensors ok")
"""


def test_torch_tensors_through_quantize_device(tmp_path):
    """a torch device tensor sliced at an odd frame (8-byte aligned) and at an even one, strided outputs (torch first in a
    process of its own: it brings its own copy of the HIP runtime)"""
    np.save(tmp_path / "level.npy", _ladder(36)[256])
    (tmp_path / "t.py").write_text(_TORCH_SCRIPT)
    r = subprocess.run([sys.executable, str(tmp_path / "t.py"), ROOT, str(tmp_path / "level.npy")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "torch tensors ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_short_strides_are_refused():
    P = 36
    with e.CodebookSet(P, _set_codebooks(P, [2, 4])) as cs:
        with pytest.raises(e.Ecoz2Error, match="strides"):
            cs.quantize_device(1 << 20, 100, 1 << 21, 99)


def _frame_of_codeword(row):
    """the frame that IS a codeword: the gain-normalised autocorrelation whose reflection coefficients are `row` (inverse
    Levinson recursion, r / prediction error) -- its distortion to that codeword is the floor, 1"""
    P = len(row) - 1
    r, a, E = np.zeros(P + 1), np.zeros(P + 1), 1.0
    r[0] = a[0] = 1.0
    for m in range(1, P + 1):
        k = row[m]
        r[m] = -(k * E + sum(a[i] * r[m - i] for i in range(1, m)))
        nxt = a.copy()
        for i in range(1, m):
            nxt[i] = a[i] + k * a[m - i]
        nxt[m] = k
        a, E = nxt, E * (1.0 - k * k)
    return r / E


@pytest.mark.parametrize("P", [36, 48])
def test_ties_take_the_lowest_index(oracle, P):
    """every codebook of the set holds its most popular codeword twice: every frame of that cell ties exactly, and the
    lower of the two indices must win, as in the single call and the oracle.  Among the frames are frames EQUAL to
    codewords (_frame_of_codeword) -- of the duplicated row, of row 0, whose padding copies beyond M (M = 5, 40, 300 are not
    multiples of 16) tie with it at the floor of the distortion, and of the last row: each must get the lowest index that
    holds its codeword."""
    lv = _ladder(P)
    plain = _frames(P, 3000, seed=21)
    cbs, pairs = [], []
    for M in (5, 16, 40, 300):
        base = lv[1 << (M - 1).bit_length()][:M].copy()
        a = int(np.bincount(_single(P, base, plain)[0], minlength=M).argmax())
        j = (a + 1 + M // 2) % M
        base[j] = base[a]
        cbs.append(base)
        pairs.append((min(a, j), max(a, j)))
    # per codebook three frames equal to codewords: the duplicated row, row 0, the last row
    own = [[pairs[k][1], 0, len(cb) - 1] for k, cb in enumerate(cbs)]
    exact = np.array([_frame_of_codeword(cb[m]) for cb, rows in zip(cbs, own) for m in rows])
    frames = np.ascontiguousarray(np.concatenate([plain[:1500], exact, plain[1500:]]))
    with e.CodebookSet(P, cbs) as cs:
        sym, dmin = cs.quantize(frames)
    for k, cb in enumerate(cbs):
        M = len(cb)
        so, do = oracle.quantize(oracle.reflections_to_cq(cb), frames)
        s1, d1 = _single(P, cb, frames)
        assert np.array_equal(sym[k], so) and np.array_equal(sym[k], s1), (P, M)
        assert np.array_equal(_bits(dmin[k]), _bits(do)) and np.array_equal(_bits(dmin[k]), _bits(d1)), (P, M)
        lo, hi = pairs[k]
        assert (sym[k] == lo).any() and not (sym[k] == hi).any(), (P, M, lo, hi)
        for q, m in enumerate(own[k]):
            t = 1500 + 3 * k + q
            first = min(i for i in range(M) if np.array_equal(cb[i], cb[m]))  # (the lowest index holding this codeword)
            assert sym[k][t] == first and abs(dmin[k][t] - 1.0) < 1e-9, (P, M, m, int(sym[k][t]), float(dmin[k][t]))


def test_routes(monkeypatch):
    frames = _frames(36, 5000)
    cbs = _set_codebooks(36)
    n_pre = sum(1 for cb in cbs if len(cb) >= 256)
    assert n_pre == 3
    with e.CodebookSet(36, cbs) as cs:
        assert cs.launch_counts() == (0, 0)
        for call in (1, 2, 3):
            cs.quantize(frames)
            # one launch of k_quantize_set per call, one group of single launches per prefiltered codebook
            assert cs.launch_counts() == (call, call * n_pre)
    with e.CodebookSet(36, [cb for cb in cbs if len(cb) < 256]) as cs:
        cs.quantize(frames)
        assert cs.launch_counts() == (1, 0)
    with e.CodebookSet(36, [cb for cb in cbs if len(cb) >= 256]) as cs:
        cs.quantize(frames)
        assert cs.launch_counts() == (0, n_pre)
    for P in (100, 48, 3):  # no narrow MFMA sweep: zero set launches
        with e.CodebookSet(P, _set_codebooks(P, [2, 16, 100]) if P != 3 else [np.eye(4)[:2] * 0.5 + 0.1]) as cs:
            cs.quantize(_frames(P, 500))
            assert cs.launch_counts()[0] == 0 and cs.launch_counts()[1] == cs.K
    # with the prefilter off every codebook of a narrow order is the set kernel's
    monkeypatch.setenv("ECOZ2_VQ_PREFILTER", "0")
    with e.CodebookSet(36, cbs) as cs:
        sym, dmin = cs.quantize(frames)
        assert cs.launch_counts() == (1, 0)
    monkeypatch.delenv("ECOZ2_VQ_PREFILTER")
    with e.CodebookSet(36, cbs) as cs:
        sym2, dmin2 = cs.quantize(frames)
    assert np.array_equal(sym, sym2) and np.array_equal(_bits(dmin), _bits(dmin2))


# ---- files -----------------------------------------------------------------------------------------------------------------
FILE_SIZES = [1, 63, 65, 700, 4000, 20000]
P_FILES = 36
FILE_MS = [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = tmp_path_factory.mktemp("qcorpus")
    files = []
    for k, f in enumerate(_class_frames(P_FILES, FILE_SIZES + [9001], seed=31)):
        name = f"C{(k * 3) % 7}"
        p = root / "data" / "predictors" / name / f"f{k:02d}.prd"
        p.parent.mkdir(parents=True, exist_ok=True)
        e.formats.write_prd(str(p), name, f)
        files.append(str(p))
    lv = _ladder(P_FILES)
    cbs = {}
    for M in FILE_MS:
        p = root / "data" / "codebooks" / "_" / f"eps_0.05_M_{M:04d}.cbook"
        p.parent.mkdir(parents=True, exist_ok=True)
        e.formats.write_cbook(str(p), "_", lv[M])
        cbs[M] = str(p)
    return root, files, cbs


def _shuffled(cbs):
    order = list(cbs)
    np.random.default_rng(3).shuffle(order)
    assert order != sorted(order)
    return [cbs[M] for M in order]


def _loop(files, cbs, out, show, monkeypatch, capfd):
    monkeypatch.setenv("ECOZ2_VQ_OUT_ROOT", str(out))
    fs, _keep = vq._to_vec_of_ptr_const_c_char(files)
    capfd.readouterr()
    for M in sorted(cbs):
        assert e.lib.ecoz2_vq_quantize(cbs[M].encode(), fs, len(files), int(show)) == 0, e.lib.e2vq_last_error()
    return _read_tree(out), capfd.readouterr().out.replace(str(out), "<out>")


def _set_call(files, cb_files, out, show, monkeypatch, capfd):
    monkeypatch.setenv("ECOZ2_VQ_OUT_ROOT", str(out))
    capfd.readouterr()
    vq.vq_quantize_codebooks(cb_files, files, show)
    return _read_tree(out), capfd.readouterr().out.replace(str(out), "<out>")


@pytest.mark.parametrize("show", [False, True])
def test_files_equal_the_loop_of_single_calls(corpus, tmp_path, monkeypatch, capfd, show):
    _root, files, cbs = corpus
    monkeypatch.setenv("ECOZ2_VQ_QUANTIZE_CHUNK", "4096")  # (the 9001- and 20000-frame files are split: .tmp + rename)
    tree1, out1 = _loop(files, cbs, tmp_path / "loop", show, monkeypatch, capfd)
    treeK, outK = _set_call(files, _shuffled(cbs), tmp_path / "set", show, monkeypatch, capfd)
    assert len(tree1) == len(FILE_MS) * len(files) and not [p for p in tree1 if p.endswith(".tmp")]
    assert sorted(treeK) == sorted(tree1)
    assert treeK == tree1
    assert outK == out1
    assert outK.count("total: ") == len(FILE_MS) and (outK.count(" -> ") == len(FILE_MS) * len(files)) == show
    Ms = [int(l.split("M=")[1].split(",")[0]) for l in outK.splitlines() if l.startswith("total: ")]
    assert Ms == sorted(FILE_MS)


@pytest.mark.parametrize("show", [False, True])
def test_files_through_the_cli(corpus, tmp_path, show):
    root, files, cbs = corpus
    env = dict(os.environ, ECOZ2_VQ_QUANTIZE_CHUNK="4096")
    flags = ["-s"] if show else []
    outs, trees = [], []
    for name, runs in (("loop", [["--codebook", cbs[M]] for M in sorted(cbs)]),
                       ("set", [["--codebooks", str(root / "data" / "codebooks")]])):
        out = tmp_path / name
        text = ""
        for args in runs:
            r = subprocess.run([CLI, "vq", "quantize", *args, *flags, "--predictors", str(root / "data" / "predictors")],
                               capture_output=True, text=True, cwd=tmp_path, env=dict(env, ECOZ2_VQ_OUT_ROOT=str(out)))
            assert r.returncode == 0 and "ERROR" not in r.stderr, r.stderr
            # (the library's lines: the CLI's own header -- file count, one nom_raas line per codebook -- comes per process)
            text += "".join(l + "\n" for l in r.stdout.splitlines()
                            if not l.startswith(("number of predictor files:", "nom_raas = ")))
        outs.append(text.replace(str(out), "<out>"))
        trees.append(_read_tree(out))
    assert trees[0] == trees[1] and len(trees[0]) == len(FILE_MS) * len(files)
    assert outs[0] == outs[1] and outs[0].count("total: ") == len(FILE_MS)
    assert (outs[0].count(" -> ") == len(FILE_MS) * len(files)) == show


def test_files_invariant_under_workers_and_chunk(corpus, tmp_path, monkeypatch, capfd):
    _root, files, cbs = corpus
    cb_files = _shuffled(cbs)
    monkeypatch.setenv("ECOZ2_VQ_QUANTIZE_CHUNK", "4096")
    monkeypatch.setenv("ECOZ2_VQ_GPUS", "1")
    ref = _set_call(files, cb_files, tmp_path / "ref", True, monkeypatch, capfd)
    n = 0
    for gpus in ("1", "2", "3"):
        for chunk in ("1024", "4096", None):
            monkeypatch.setenv("ECOZ2_VQ_GPUS", gpus)
            if chunk:
                monkeypatch.setenv("ECOZ2_VQ_QUANTIZE_CHUNK", chunk)
            else:
                monkeypatch.delenv("ECOZ2_VQ_QUANTIZE_CHUNK", raising=False)
            n += 1
            assert _set_call(files, cb_files, tmp_path / f"v{n}", True, monkeypatch, capfd) == ref, (gpus, chunk)


def test_nan_in_a_late_frame_fails_and_leaves_no_tmp(corpus, tmp_path, monkeypatch):
    _root, files, cbs = corpus
    frames = _class_frames(P_FILES, [9000], seed=2)[0]
    frames[8500, 7] = np.nan
    bad = tmp_path / "bad_late.prd"
    e.formats.write_prd(str(bad), "C9", frames)
    out = tmp_path / "out"
    monkeypatch.setenv("ECOZ2_VQ_OUT_ROOT", str(out))
    monkeypatch.setenv("ECOZ2_VQ_QUANTIZE_CHUNK", "1024")
    with pytest.raises(e.Ecoz2Error, match="bad_late.prd"):
        vq.vq_quantize_codebooks([cbs[4], cbs[512], cbs[64]], files[:3] + [str(bad)], False)
    assert not list(out.rglob("*.tmp"))
    assert not list(out.rglob("bad_late.seq"))


def test_trees_feed_hmm_learn_grid(corpus, tmp_path, monkeypatch, capfd):
    _root, files, cbs = corpus
    out = tmp_path / "out"
    monkeypatch.setenv("ECOZ2_VQ_OUT_ROOT", str(out))
    monkeypatch.setenv("ECOZ2_VQ_QUIET", "1")
    files = files[1:]  # (without the one-frame file)
    vq.vq_quantize_codebooks([cbs[16], cbs[4]], files, False)
    seqs = sorted(str(p) for p in (out / "data" / "sequences").rglob("*.seq"))
    assert len(seqs) == 2 * len(files)
    e.hmm.set_random_seed(11)
    e.hmm.hmm_learn_grid([3], 3, seqs, 1e-5, 0.3, 2)
    classes = {e.formats.read_prd(f)[0] for f in files}
    shapes = sorted(e.hmm.load_model(str(p))[3].shape for p in out.rglob("*.hmm"))
    assert shapes == [(3, 4)] * len(classes) + [(3, 16)] * len(classes)
