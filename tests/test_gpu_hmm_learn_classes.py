"""`hmm learn --all-classes` on the GPU: every class's model trained in one batched training must be
the single-class training's, bit for bit -- on arrays (e2vq_hmm_train_classes against e2vq_hmm_train and the oracle),
on files (e2vq_hmm_learn_classes against a loop of seeded ecoz2_hmm_learn calls: .hmm, .csv, stdout, callbacks, the
generator state after the call), for any ECOZ2_VQ_GPUS and any ECOZ2_HMM_LEARN_BATCH_BYTES, and through the CLI."""
import os
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from tests import oracle_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    return oracle_lib.load_hmm()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _class_seqs(rng, M, sizes, bad_class):
    """len(sizes) classes of ragged sequences drawn around a per-class drift; class 1 holds an empty and a one-symbol
    sequence, class `bad_class` a sequence that starts with symbol 0 (which its initial model cannot emit at t = 0)"""
    out = []
    for k, S_k in enumerate(sizes):
        seqs = []
        for q in range(S_k):
            T = int(rng.integers(2, 40))
            base = (np.linspace(0, M - 1, T) * (1 + k % 3) / 3 + k)
            s = np.clip((base + rng.normal(0, M / 6, T)).round(), 1, M - 1).astype(np.uint16) % M
            s[s == 0] = 1
            seqs.append(s)
        if k == 1:
            seqs[0] = np.zeros(0, dtype=np.uint16)
            if S_k > 1:
                seqs[1] = np.array([3 % M], dtype=np.uint16)
        if k == bad_class:
            seqs[-1] = np.concatenate([[0], seqs[-1]]).astype(np.uint16)
        out.append(seqs)
    return out


def _models(H, K, N, M, typ, bad_class):
    ms = []
    for k in range(K):
        pi, A, B = H.init(N, M, typ)
        if k == bad_class:  # state 0 (the start state of the cascades) cannot emit symbol 0
            B = B.copy()
            B[0, 0] = 0.0
            B[0] /= B[0].sum()
        ms.append((pi, A, B))
    return ms


SIZES = [1, 3, 9, 2, 17, 5, 40]  # K = 7 classes, unequal S_k, one of them a single sequence


@pytest.mark.parametrize("N", [1, 5, 64, 65, 141, 142])
@pytest.mark.parametrize("typ", [0, 1, 2, 3])
def test_train_classes_equals_single_training(H, N, typ):
    M = 16 if N > 64 else 32
    maxit = 4 if N > 64 else 12
    H.seed(1000 + 7 * N + typ)
    rng = np.random.default_rng(N * 10 + typ)
    bad = 5
    cls = _class_seqs(rng, M, SIZES, bad)
    models = _models(H, len(SIZES), N, M, typ, bad)
    got = e.hmm.train_classes(models, cls, 1e-5, 0.3, maxit)
    assert len(got) == len(SIZES)
    for k, (m, seqs) in enumerate(zip(models, cls)):
        pg, Ag, Bg, hist = e.hmm.train(*m, seqs, 1e-5, 0.3, maxit)
        pb, Ab, Bb, hist_b = got[k]
        assert hist_b == hist and 1 <= len(hist) <= maxit, k
        for a, b in ((pg, pb), (Ag, Ab), (Bg, Bb)):
            assert np.array_equal(_bits(a), _bits(b)), k
        if k in (0, 3, bad) and (N <= 65 or k == 0):  # a subset against the oracle (no empty sequence there)
            po, Ao, Bo, hist_o = H.learn(*m, seqs, 1e-5, 0.3, maxit)
            assert hist_o == hist_b
            for a, b in ((po, pb), (Ao, Ab), (Bo, Bb)):
                assert np.array_equal(_bits(a), _bits(b)), k
    # the unemittable sequence was skipped: its class's training still ran
    assert got[bad][3] and np.isfinite(got[bad][3][0])


@pytest.mark.parametrize("N", [4, 70])
@pytest.mark.parametrize("val_auto,maxit", [(2.0, -1), (0.05, -1), (0.3, 0), (0.3, 1), (0.3, 2)])
def test_classes_stop_at_their_own_iteration(H, N, val_auto, maxit):
    M = 24
    H.seed(77 + N)
    rng = np.random.default_rng(5 + N)
    sizes = [6, 30, 2, 12, 20, 1]
    cls = _class_seqs(rng, M, sizes, -1)
    models = _models(H, len(sizes), N, M, 0, -1)
    fixed = maxit >= 0
    if N > 64 and maxit < 0:
        maxit = 6  # (the workgroup kernel: a bound on the iterations, the classes may still stop earlier)
    got = e.hmm.train_classes(models, cls, 0.0, val_auto, maxit)
    lens = []
    for k, (m, seqs) in enumerate(zip(models, cls)):
        pg, Ag, Bg, hist = e.hmm.train(*m, seqs, 0.0, val_auto, maxit)
        assert got[k][3] == hist, k
        for a, b in zip((pg, Ag, Bg), got[k][:3]):
            assert np.array_equal(_bits(a), _bits(b)), k
        lens.append(len(hist))
    if fixed:
        assert set(lens) == {maxit}
    elif N <= 64:
        assert len(set(lens)) >= 2, lens  # (the point of the case: classes stop at different iterations)


def test_train_classes_batch_budget_is_invisible(H, monkeypatch):
    H.seed(9)
    rng = np.random.default_rng(9)
    cls = _class_seqs(rng, 32, [4, 7, 1, 11, 3], -1)
    models = _models(H, 5, 6, 32, 3, -1)
    one = e.hmm.train_classes(models, cls, 1e-5, 0.3, -1)
    monkeypatch.setenv("ECOZ2_HMM_LEARN_BATCH_BYTES", "1")  # every class a batch of its own
    many = e.hmm.train_classes(models, cls, 1e-5, 0.3, -1)
    for a, b in zip(one, many):
        assert a[3] == b[3] and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[:3], b[:3]))


# ---- files ---------------------------------------------------------------------------------------------------------------
def _file_corpus(root, n_classes=20, M=64, seed=11):
    """a self-contained 20-class corpus: class c's sequences follow a random Markov chain over the M symbols with a
    sharp preferred successor per symbol; the list interleaves the classes (so grouping keeps list order per class)"""
    rng = np.random.default_rng(seed)
    per_class = {}
    for c in range(n_classes):
        succ = rng.permutation(M)
        name = f"K{(c * 7) % n_classes:02d}"  # (names out of creation order)
        files = []
        for q in range(int(rng.integers(4, 14))):
            T = int(rng.integers(15, 70))
            s = np.zeros(T, dtype=np.uint16)
            s[0] = rng.integers(0, M)
            for t in range(1, T):
                s[t] = succ[s[t - 1]] if rng.random() < 0.7 else rng.integers(0, M)
            p = root / "seqs" / name / f"{q:03d}.seq"
            p.parent.mkdir(parents=True, exist_ok=True)
            e.formats.write_seq(str(p), name, M, s)
            files.append(str(p))
        per_class[name] = files
    order = []
    while any(per_class.values()):
        for name in list(per_class):
            if per_class[name]:
                order.append(per_class[name].pop(int(rng.integers(0, len(per_class[name])))))
    return order


def _read_tree(d):
    return {str(p.relative_to(d)): p.read_bytes() for p in sorted(d.rglob("*")) if p.is_file()}


def _single_loop(files, out, monkeypatch, capfd, N, typ, seed, eps, auto, maxit):
    monkeypatch.setenv("ECOZ2_VQ_OUT_ROOT", str(out))
    by_class = {}
    for f in files:
        by_class.setdefault(e.formats.read_seq(f)[0], []).append(f)
    seen, blocks = [], []
    capfd.readouterr()
    for name in sorted(by_class, key=lambda s: s.encode()):
        e.hmm.set_random_seed(seed)
        e.hmm.hmm_learn(N, typ, by_class[name], eps, auto, maxit, callback=lambda v, x: seen.append((v, x)))
        blocks.append(capfd.readouterr().out)
    after = e.hmm.init_model(2, 8, 0)  # (the generator's next draw after the last call)
    return _read_tree(out), seen, "".join(blocks), len(by_class), after


def _batched(files, out, monkeypatch, capfd, N, typ, seed, eps, auto, maxit):
    monkeypatch.setenv("ECOZ2_VQ_OUT_ROOT", str(out))
    seen = []
    capfd.readouterr()
    e.hmm.set_random_seed(seed)
    e.hmm.hmm_learn_classes(N, typ, files, eps, auto, maxit, callback=lambda v, x: seen.append((v, x)))
    text = capfd.readouterr().out
    after = e.hmm.init_model(2, 8, 0)
    return _read_tree(out), seen, text, after


@pytest.mark.parametrize("N,typ,maxit", [(5, 3, -1), (3, 0, 7), (70, 2, 2)])
def test_learn_classes_files_equal_the_single_loop(tmp_path, monkeypatch, capfd, N, typ, maxit):
    monkeypatch.delenv("ECOZ2_VQ_QUIET", raising=False)
    monkeypatch.setenv("ECOZ2_VQ_GPUS", "1")
    files = _file_corpus(tmp_path)
    tree1, seen1, text1, K, after1 = _single_loop(files, tmp_path / "one", monkeypatch, capfd, N, typ, 1234, 1e-5, 0.3, maxit)
    tree2, seen2, text2, after2 = _batched(files, tmp_path / "all", monkeypatch, capfd, N, typ, 1234, 1e-5, 0.3, maxit)
    assert K == 20 and len(tree1) == 2 * K
    assert tree1.keys() == tree2.keys()
    for k in tree1:
        assert tree1[k] == tree2[k], k
    assert seen2 == seen1 and len(seen1) >= K
    assert text2.replace(str(tmp_path / "all"), "@") == text1.replace(str(tmp_path / "one"), "@")
    assert text2.count("HMM learn: class '") == K and "  it=0  sum log(P) = " in text2
    for a, b in zip(after1, after2):  # the generator is left where a single call leaves it
        assert np.array_equal(_bits(a), _bits(b))


def test_learn_classes_invariant_to_workers_and_batches(tmp_path, monkeypatch, capfd):
    monkeypatch.setenv("ECOZ2_VQ_QUIET", "1")
    files = _file_corpus(tmp_path, seed=12)
    runs = []
    for i, (gpus, budget) in enumerate([("1", None), ("2", None), ("3", None), ("1", "1"), ("3", "200000")]):
        monkeypatch.setenv("ECOZ2_VQ_GPUS", gpus)
        if budget:
            monkeypatch.setenv("ECOZ2_HMM_LEARN_BATCH_BYTES", budget)  # "1": 20 batches; 200 000: several classes each
        else:
            monkeypatch.delenv("ECOZ2_HMM_LEARN_BATCH_BYTES", raising=False)
        tree, seen, text, _after = _batched(files, tmp_path / f"r{i}", monkeypatch, capfd, 5, 3, 99, 1e-5, 0.3, -1)
        runs.append((tree, seen, text.replace(str(tmp_path / f"r{i}"), "@")))
    for r in runs[1:]:
        assert r == runs[0]


def test_learn_classes_cli(tmp_path):
    exe = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
    env = dict(os.environ, NO_COLOR="1")
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_QUIET", "ECOZ2_HMM_LEARN_BATCH_BYTES", "ECOZ2_VQ_GPUS"):
        env.pop(k, None)
    rng = np.random.default_rng(4)
    rows, classes = ["tt,class,selection"], ["C00", "C01", "C02"]
    for c, cls in enumerate(classes):
        for k in range(9):
            s = np.clip((np.linspace(0, 31, 40) + 6 * c + rng.normal(0, 3, 40)).round(), 0, 31).astype(np.uint16)
            p = tmp_path / "data" / "sequences" / "M32" / cls / f"{k:05d}.seq"
            p.parent.mkdir(parents=True, exist_ok=True)
            e.formats.write_seq(str(p), cls, 32, s)
            rows.append(f"{'TRAIN' if k < 6 else 'TEST'},{cls},{k:05d}")
    (tmp_path / "tt.csv").write_text("\n".join(rows) + "\n")

    def run(root, *args):
        r = subprocess.run([exe, *args], cwd=tmp_path, env=dict(env, ECOZ2_VQ_OUT_ROOT=str(tmp_path / root)),
                           capture_output=True, text=True, timeout=600)
        return r.returncode, r.stdout, r.stderr

    for cls in classes:
        rc, out, err = run("one", "hmm", "learn", "-N", "4", "-M", "32", "-s", "3", "-I", "8", "--class-name", cls,
                           "--sequences", "tt.csv")
        assert rc == 0, err
    rc, out, err = run("all", "hmm", "learn", "--all-classes", "-N", "4", "-M", "32", "-s", "3", "-I", "8",
                       "--sequences", "tt.csv")
    assert rc == 0, err
    head = out.split("\n")
    assert head[1:4] == ["sequences: 18", "classes: 3", "val_auto = 0.3"] and head[0].startswith("ECOZ2 C version")
    assert out.count("model saved: ") == 3
    one, all_ = _read_tree(tmp_path / "one"), _read_tree(tmp_path / "all")
    assert len(one) == 6 and one == all_
    rc, out, err = run("bad", "hmm", "learn", "--all-classes", "--class-name", "C00", "-M", "32", "--sequences", "tt.csv")
    assert rc == 2 and "exclude each other" in err and not (tmp_path / "bad").exists()
