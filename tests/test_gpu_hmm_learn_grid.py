"""`hmm learn --grid` on the GPU: every (N, M, class) model trained in one batched training must be the
single training's, bit for bit -- on arrays (e2vq_hmm_train_grid against e2vq_hmm_train and the oracle, across both
E-step paths, overlapping sequence ranges and models that stop at different iterations), on files (e2vq_hmm_learn_grid
against a loop of seeded e2vq_hmm_learn_classes calls, one per (N, M): .hmm, .csv, stdout, callbacks, the generator state
after the call), for any ECOZ2_VQ_GPUS and ECOZ2_HMM_LEARN_BATCH_BYTES, and through the CLI.
e2vq_hmm_learn_classes runs on the same batched trainer as the grid, so the file comparisons show that one grid call
equals many one-(N, M) calls of it, not that either is right: the independent reference is the single-class training
(the array tests here, and test_gpu_hmm_learn_classes.py against seeded ecoz2_hmm_learn loops)."""
import os
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from tests import oracle_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")


@pytest.fixture(scope="module")
def H():
    return oracle_lib.load_hmm()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _grid_case(H, Ns, Ms, sizes, typ, seed):
    """per M: len(sizes) classes of ragged sequences (class 1 holds an empty sequence; the last class of each M a
    sequence that starts with symbol 0, which its initial models cannot emit at t = 0); one model per (N, M, class)
    in grid order, plus per M one model of the smallest N over classes 0 and 1 together (a range that overlaps others)"""
    rng = np.random.default_rng(seed)
    H.seed(seed)
    seqs, ranges, models, bad = [], [], [], set()
    cls_ranges = {}
    for M in Ms:
        for k, S_k in enumerate(sizes):
            lo = len(seqs)
            for q in range(S_k):
                T = int(rng.integers(2, 30))
                s = np.clip((np.linspace(0, M - 1, T) * (1 + k % 3) / 3 + k + rng.normal(0, M / 6, T)).round(), 1, M - 1)
                seqs.append(s.astype(np.uint16))
            if k == 1:
                seqs[lo] = np.zeros(0, dtype=np.uint16)
            if k == len(sizes) - 1:
                seqs[-1] = np.concatenate([[0], seqs[-1]]).astype(np.uint16)
            cls_ranges[(M, k)] = (lo, len(seqs))
    for N in Ns:
        for M in Ms:
            for k in range(len(sizes)):
                pi, A, B = H.init(N, M, typ)
                if k == len(sizes) - 1:  # state 0 (the start state of the cascades) cannot emit symbol 0
                    B = B.copy()
                    B[0, 0] = 0.0
                    B[0] /= B[0].sum()
                    bad.add(len(models))
                models.append((pi, A, B))
                ranges.append(cls_ranges[(M, k)])
    for M in Ms:
        models.append(H.init(Ns[0], M, typ))
        ranges.append((cls_ranges[(M, 0)][0], cls_ranges[(M, 1)][1]))
    return models, seqs, ranges, bad


@pytest.mark.parametrize("typ", [0, 3])
def test_train_grid_equals_single_training(H, typ):
    Ns, Ms = [1, 5, 64, 65, 70], [8, 33, 256]
    models, seqs, ranges, bad = _grid_case(H, Ns, Ms, [3, 6, 2], typ, 500 + typ)
    maxit, auto = 5, 0.05
    got = e.hmm.train_grid(models, seqs, ranges, 1e-5, auto, maxit)
    assert len(got) == len(models)
    lens = set()
    for k, (m, (lo, hi)) in enumerate(zip(models, ranges)):
        pg, Ag, Bg, hist = e.hmm.train(*m, seqs[lo:hi], 1e-5, auto, maxit)
        pb, Ab, Bb, hist_b = got[k]
        assert hist_b == hist and 1 <= len(hist) <= maxit, k
        lens.add(len(hist))
        for a, b in ((pg, pb), (Ag, Ab), (Bg, Bb)):
            assert np.array_equal(_bits(a), _bits(b)), k
        if k % 7 == 0 and len(m[0]) <= 65 and all(len(s) for s in seqs[lo:hi]):  # a subset against the oracle
            po, Ao, Bo, hist_o = H.learn(*m, seqs[lo:hi], 1e-5, auto, maxit)
            assert hist_o == hist_b, k
            for a, b in ((po, pb), (Ao, Ab), (Bo, Bb)):
                assert np.array_equal(_bits(a), _bits(b)), k
    assert len(lens) >= 2, lens  # (models stop at different iterations)
    for k in bad:  # the unemittable sequence was skipped: the model still trained
        assert got[k][3] and np.isfinite(got[k][3][0])


def test_train_grid_oracle_on_shared_sequences(H):
    """models of several N on one set of sequences (every range the same), checked against the oracle directly"""
    rng = np.random.default_rng(8)
    seqs = [rng.integers(0, 12, int(rng.integers(5, 40))).astype(np.uint16) for _ in range(9)]
    H.seed(8)
    models = [H.init(N, 12, 0) for N in (2, 7, 64, 66)]
    got = e.hmm.train_grid(models, seqs, [(0, 9)] * 4, 1e-5, 0.3, 4)
    for m, g in zip(models, got):
        po, Ao, Bo, hist_o = H.learn(*m, seqs, 1e-5, 0.3, 4)
        assert g[3] == hist_o
        for a, b in zip((po, Ao, Bo), g[:3]):
            assert np.array_equal(_bits(a), _bits(b))


def test_train_grid_batch_budget_is_invisible(H, monkeypatch):
    models, seqs, ranges, _bad = _grid_case(H, [3, 6, 65], [16, 40], [4, 3, 5], 3, 9)
    one = e.hmm.train_grid(models, seqs, ranges, 1e-5, 0.3, 4)
    for budget in ("1", "40000"):  # every model a batch of its own; a few models each
        monkeypatch.setenv("ECOZ2_HMM_LEARN_BATCH_BYTES", budget)
        many = e.hmm.train_grid(models, seqs, ranges, 1e-5, 0.3, 4)
        for a, b in zip(one, many):
            assert a[3] == b[3] and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[:3], b[:3]))


# ---- files ---------------------------------------------------------------------------------------------------------------
def _file_corpus(root, Ms, seed=11):
    """per M a self-contained corpus of 4 to 6 classes (random Markov chains over the M symbols); the list interleaves
    the M values and the classes"""
    rng = np.random.default_rng(seed)
    files = []
    for M in Ms:
        for c in range(int(rng.integers(4, 7))):
            succ = rng.permutation(M)
            name = f"K{(c * 3) % 7:02d}"
            for q in range(int(rng.integers(3, 9))):
                T = int(rng.integers(15, 50))
                s = np.zeros(T, dtype=np.uint16)
                s[0] = rng.integers(0, M)
                for t in range(1, T):
                    s[t] = succ[s[t - 1]] if rng.random() < 0.7 else rng.integers(0, M)
                p = root / "seqs" / f"M{M}" / name / f"{q:03d}.seq"
                p.parent.mkdir(parents=True, exist_ok=True)
                e.formats.write_seq(str(p), name, M, s)
                files.append(str(p))
    return [files[i] for i in rng.permutation(len(files))]


def _read_tree(d):
    return {str(p.relative_to(d)): p.read_bytes() for p in sorted(d.rglob("*")) if p.is_file()}


def _loop(files, Ns, out, monkeypatch, capfd, typ, seed, eps, auto, maxit):
    """seeded e2vq_hmm_learn_classes once per (N, M), in grid order"""
    monkeypatch.setenv("ECOZ2_VQ_OUT_ROOT", str(out))
    by_M = {}
    for f in files:
        by_M.setdefault(e.formats.read_seq(f)[1], []).append(f)
    seen, blocks = [], []
    capfd.readouterr()
    for N in sorted(Ns):
        for M in sorted(by_M):
            e.hmm.set_random_seed(seed)
            e.hmm.hmm_learn_classes(N, typ, by_M[M], eps, auto, maxit, callback=lambda v, x: seen.append((v, x)))
            blocks.append(capfd.readouterr().out)
    after = e.hmm.init_model(2, 8, 0)  # (the generator's next draw after the last call)
    return _read_tree(out), seen, "".join(blocks), after


def _grid(files, Ns, out, monkeypatch, capfd, typ, seed, eps, auto, maxit):
    monkeypatch.setenv("ECOZ2_VQ_OUT_ROOT", str(out))
    seen = []
    capfd.readouterr()
    e.hmm.set_random_seed(seed)
    e.hmm.hmm_learn_grid(Ns, typ, files, eps, auto, maxit, callback=lambda v, x: seen.append((v, x)))
    text = capfd.readouterr().out
    after = e.hmm.init_model(2, 8, 0)
    return _read_tree(out), seen, text, after


@pytest.mark.parametrize("Ns,typ,maxit", [([5, 3], 3, -1), ([2, 64, 65], 0, 3)])
def test_learn_grid_files_equal_the_loop(tmp_path, monkeypatch, capfd, Ns, typ, maxit):
    monkeypatch.delenv("ECOZ2_VQ_QUIET", raising=False)
    monkeypatch.setenv("ECOZ2_VQ_GPUS", "1")
    files = _file_corpus(tmp_path, [16, 33, 64])
    tree1, seen1, text1, after1 = _loop(files, Ns, tmp_path / "one", monkeypatch, capfd, typ, 1234, 1e-5, 0.3, maxit)
    tree2, seen2, text2, after2 = _grid(files, Ns, tmp_path / "all", monkeypatch, capfd, typ, 1234, 1e-5, 0.3, maxit)
    assert len(tree1) >= 2 * 3 * len(Ns) * 4
    assert tree1.keys() == tree2.keys()
    for k in tree1:
        assert tree1[k] == tree2[k], k
    assert seen2 == seen1 and len(seen1) >= len(tree1) // 2
    assert text2.replace(str(tmp_path / "all"), "@") == text1.replace(str(tmp_path / "one"), "@")
    assert "  it=0  sum log(P) = " in text2
    for a, b in zip(after1, after2):  # the generator is left where a seeded single call for the last model leaves it
        assert np.array_equal(_bits(a), _bits(b))


def test_learn_grid_invariant_to_workers_and_batches(tmp_path, monkeypatch, capfd):
    monkeypatch.setenv("ECOZ2_VQ_QUIET", "1")
    files = _file_corpus(tmp_path, [16, 40], seed=12)
    runs = []
    for i, (gpus, budget) in enumerate([("1", None), ("2", None), ("3", None), ("1", "1"), ("3", "60000")]):
        monkeypatch.setenv("ECOZ2_VQ_GPUS", gpus)
        if budget:
            monkeypatch.setenv("ECOZ2_HMM_LEARN_BATCH_BYTES", budget)
        else:
            monkeypatch.delenv("ECOZ2_HMM_LEARN_BATCH_BYTES", raising=False)
        tree, seen, text, after = _grid(files, [4, 66], tmp_path / f"r{i}", monkeypatch, capfd, 3, 99, 1e-5, 0.3, 3)
        runs.append((tree, seen, text.replace(str(tmp_path / f"r{i}"), "@"), [_bits(x).tolist() for x in after]))
    for r in runs[1:]:
        assert r == runs[0]


# ---- CLI -----------------------------------------------------------------------------------------------------------------
def _cli_tree(tmp_path):
    rng = np.random.default_rng(4)
    rows = ["tt,class,selection"]
    classes = ["C00", "C01", "C02"]
    for c, cls in enumerate(classes):
        for k in range(7):
            rows.append(f"{'TRAIN' if k < 5 else 'TEST'},{cls},{k:05d}")
            for M in (16, 33):
                s = np.clip((np.linspace(0, M - 1, 30) + 4 * c + rng.normal(0, 3, 30)).round(), 0, M - 1).astype(np.uint16)
                p = tmp_path / "data" / "sequences" / f"M{M}" / cls / f"{k:05d}.seq"
                p.parent.mkdir(parents=True, exist_ok=True)
                e.formats.write_seq(str(p), cls, M, s)
    (tmp_path / "tt.csv").write_text("\n".join(rows) + "\n")


@pytest.mark.parametrize("source", ["csv", "dirs"])
def test_learn_grid_cli_equals_all_classes_runs(tmp_path, source):
    env = dict(os.environ, NO_COLOR="1")
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_QUIET", "ECOZ2_HMM_LEARN_BATCH_BYTES", "ECOZ2_VQ_GPUS"):
        env.pop(k, None)
    _cli_tree(tmp_path)

    def run(root, *args):
        r = subprocess.run([EXE, "hmm", "learn", *args], cwd=tmp_path, env=dict(env, ECOZ2_VQ_OUT_ROOT=str(tmp_path / root)),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout.replace(str(tmp_path / root), "@")

    src = lambda M: ["tt.csv"] if source == "csv" else [f"data/sequences/M{M}"]
    blocks = ""
    for N in (3, 5, 65):
        for M in (16, 33):
            out = run("one", "--all-classes", "-N", str(N), "-M", str(M), "-s", "7", "-I", "4", "--sequences", *src(M))
            blocks += out[out.index("\nHMM learn: "):]
    grid_src = ["tt.csv"] if source == "csv" else ["data/sequences/M33", "data/sequences/M16"]
    out = run("grid", "--grid", "-N", "65,3,5", "-M", "33,16", "-s", "7", "-I", "4", "--sequences", *grid_src)
    head = out.split("\n")
    n_seq = 30 if source == "csv" else 42
    assert head[0].startswith("ECOZ2 C version") and head[1:5] == [f"sequences: {n_seq}", "classes: 3", "grid: N=3,5,65 M=16,33",
                                                                  "val_auto = 0.3"]
    assert out[out.index("\nHMM learn: "):] == blocks
    assert out.count("model saved: ") == 18
    one, grid = _read_tree(tmp_path / "one"), _read_tree(tmp_path / "grid")
    assert len(one) == 36 and one == grid
