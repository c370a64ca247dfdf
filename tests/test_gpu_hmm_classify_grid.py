"""`hmm classify --grid` on the GPU: every score of the batched grid scoring must be the single
scoring's, bit for bit -- on arrays (e2vq_hmm_score_grid against e2vq_hmm_score, the unchanged k_hmm_score /
k_hmm_score_wg, and a subset against the oracle: every pack width, tail packs, segments that stop alone, symbols outside
the alphabet, overlapping ranges), on files (e2vq_hmm_classify_grid against one ecoz2_hmm_classify call per point: stdout,
per-point CSV, summary), for any ECOZ2_VQ_GPUS, and through the CLI."""
import os
import re
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


def _width(N):
    return 64 // N if N <= 32 else 1


def _counts(N):
    """models per M: a multiple of the pack width, one more (a tail pack of a single model), and a short pack"""
    G = _width(N)
    return (G, G + 1, 2) if G > 1 else (2, 3, 1)


def _score_case(H, Ns, Ms, seed):
    """per M a set of sequences: the lengths 0, 1, 63, 64, 65, 128, ragged ones up to 300, one that starts with symbol 0,
    two that hold a symbol >= M (at t = 0 and at t = 70); per (N, M) _counts(N) cascade models -- every third cannot emit
    symbol 0 from its start state (status 1 at t = 0 for the sequence that starts with it), every fourth cannot emit
    symbol 3 at all (status 1 wherever a sequence first holds it) -- on the whole range of M for even positions of N in
    Ns and on an inner part of it for odd ones (ranges of different N overlap); plus one model of M = max(Ms) over all
    the sequences"""
    rng = np.random.default_rng(seed)
    H.seed(seed)
    seqs, m_range = [], {}
    for M in Ms:
        lo = len(seqs)
        for T in (0, 1, 63, 64, 65, 128, 200, 300, 17, 91, 150, 257):
            seqs.append(rng.integers(1, M, T).astype(np.uint16))
        seqs.append(np.concatenate([[0], rng.integers(1, M, 40)]).astype(np.uint16))
        bad0 = rng.integers(1, M, 30).astype(np.uint16)
        bad0[0] = M
        bad70 = rng.integers(1, M, 100).astype(np.uint16)
        bad70[70] = M
        seqs += [bad0, bad70]
        m_range[M] = (lo, len(seqs))
    models, ranges = [], []
    for q, N in enumerate(Ns):
        for M, count in zip(Ms, _counts(N)):
            lo, hi = m_range[M]
            r = (lo, hi) if q % 2 == 0 else (lo + 2, hi - 1)
            for k in range(count):
                pi, A, B = H.init(N, M, 3)
                B = B.copy()
                if k % 3 == 2:
                    B[0, 0] = 0.0
                    B[0] /= B[0].sum()
                if k % 4 == 1:
                    B[:, 3] = 0.0
                    B /= B.sum(axis=1, keepdims=True)
                models.append((pi, A, B))
                ranges.append(r)
    models.append(H.init(5, max(Ms), 0))
    ranges.append((0, len(seqs)))
    return models, seqs, ranges


def _check_against_single(models, seqs, ranges, got):
    """per group of consecutive models of one (N, M, range): one e2vq_hmm_score call (the parent's kernels)"""
    seen = set()
    k0 = 0
    while k0 < len(models):
        key = (len(models[k0][0]), models[k0][2].shape[1], ranges[k0])
        k1 = k0
        while k1 < len(models) and (len(models[k1][0]), models[k1][2].shape[1], ranges[k1]) == key:
            k1 += 1
        lo, hi = ranges[k0]
        ref = e.hmm.score(models[k0:k1], seqs[lo:hi])
        for k in range(k0, k1):
            g = got[k]
            assert np.array_equal(g["status"], ref["status"][:, k - k0]), (key, k - k0)
            assert np.array_equal(g["exp2"], ref["exp2"][:, k - k0]), (key, k - k0)
            assert np.array_equal(_bits(g["mant"]), _bits(ref["mant"][:, k - k0])), (key, k - k0)
            assert np.array_equal(_bits(g["log_prob"]), _bits(ref["log_prob"][:, k - k0])), (key, k - k0)
            seen.update((key[0], int(s)) for s in g["status"])
        k0 = k1
    return seen


@pytest.mark.parametrize("pack", [None, "1"])
def test_score_grid_equals_single_scoring(H, monkeypatch, pack):
    """pack None: the widths in use (floor(64 / N) models a wave up to N = 21, one above); "1": floor(64 / N) up to
    N = 32, so that two models to a wave (N = 22, 32) run as well"""
    monkeypatch.delenv("ECOZ2_HMM_SCORE_PACK", raising=False)
    if pack:
        monkeypatch.setenv("ECOZ2_HMM_SCORE_PACK", pack)
    Ns, Ms = [1, 2, 3, 5, 7, 16, 21, 22, 32, 33, 64, 65, 70], [8, 33, 256]
    models, seqs, ranges = _score_case(H, Ns, Ms, 41)
    got = e.hmm.score_grid(models, seqs, ranges)
    assert len(got) == len(models)
    seen = _check_against_single(models, seqs, ranges, got)
    for N in Ns:  # every status occurred at every N
        assert {(N, 0), (N, 1), (N, 2)} <= seen, N
    # a stopped segment sits among segments that went on: in some pack of N = 5 one model has status 1 on a sequence
    # that its neighbours score
    k5 = [k for k, m in enumerate(models[:-1]) if len(m[0]) == 5 and m[2].shape[1] == 8]
    st = np.stack([got[k]["status"] for k in k5])
    assert ((st == 1).any(axis=0) & (st == 0).any(axis=0)).any()
    # an empty sequence scores 0.5 * 2^1 with status 0
    assert got[0]["mant"][0] == 0.5 and got[0]["exp2"][0] == 1 and got[0]["status"][0] == 0
    # a subset against the oracle
    for k in range(0, len(models), 7):
        lo, hi = ranges[k]
        for q in range(lo, hi, 3):
            st_o, m_o, ex_o = H.forward(*models[k], seqs[q])
            g = got[k]
            assert (int(g["status"][q - lo]), float(g["mant"][q - lo]), int(g["exp2"][q - lo])) == (st_o, m_o, ex_o), (k, q)


def test_score_grid_one_model_per_wave_is_the_same(H, monkeypatch):
    """ECOZ2_HMM_SCORE_PACK=0 (the kernel's G = 1 body at every N <= 64) gives the same bits"""
    monkeypatch.delenv("ECOZ2_HMM_SCORE_PACK", raising=False)
    models, seqs, ranges = _score_case(H, [3, 5, 16, 40], [8, 33, 256], 43)
    packed = e.hmm.score_grid(models, seqs, ranges)
    monkeypatch.setenv("ECOZ2_HMM_SCORE_PACK", "0")
    single = e.hmm.score_grid(models, seqs, ranges)
    _check_against_single(models, seqs, ranges, single)
    for a, b in zip(packed, single):
        assert all(np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)) for f in ("mant", "exp2", "status", "log_prob"))


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


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """sequences of M = 16, 33, 64 and the models hmm_learn_grid trains on them for N = 3, 5, 40; both lists shuffled"""
    root = tmp_path_factory.mktemp("classify_grid")
    seq_files = _file_corpus(root, [16, 33, 64])
    old = {k: os.environ.get(k) for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_QUIET")}
    os.environ.update(ECOZ2_VQ_OUT_ROOT=str(root / "trained"), ECOZ2_VQ_QUIET="1")
    try:
        e.hmm.set_random_seed(5)
        e.hmm.hmm_learn_grid([3, 5, 40], 3, seq_files, 1e-5, 0.3, 2)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    model_files = sorted(str(p) for p in (root / "trained").rglob("*.hmm"))
    rng = np.random.default_rng(2)
    model_files = [model_files[i] for i in rng.permutation(len(model_files))]
    assert len(model_files) >= 3 * 3 * 4
    return root, model_files, seq_files


def _points(model_files, seq_files):
    """{(N, M): (models in list order, sequences in list order)}, in point order"""
    by = {}
    for f in model_files:
        _cls, pi, _A, B = e.hmm.load_model(f)
        by.setdefault((len(pi), B.shape[1]), []).append(f)
    return {(N, M): (by[(N, M)], [f for f in seq_files if e.formats.read_seq(f)[1] == M]) for N, M in sorted(by)}


def _single_calls(points, out, ranked, capfd):
    texts = {}
    capfd.readouterr()
    for (N, M), (ms, ss) in points.items():
        e.hmm.hmm_classify_sequences(ms, ss, ranked, out / f"N{N}__M{M}.csv")
        texts[(N, M)] = capfd.readouterr().out.replace(str(out), "@")
    return texts


def _grid_call(model_files, seq_files, out, ranked, capfd):
    capfd.readouterr()
    e.hmm.hmm_classify_grid(model_files, seq_files, ranked, out, out / "summary.csv")
    return capfd.readouterr().out.replace(str(out), "@")


def _split(text):
    """the grid call's stdout -> ({(N, M): the slice after its `grid point:` line}, the summary block)"""
    head, summary = text.split("\ngrid summary: ", 1)
    parts = re.split(r"^grid point: N=(\d+) M=(\d+)\n", head, flags=re.M)
    assert parts[0] == ""
    return {(int(parts[i]), int(parts[i + 1])): parts[i + 2] for i in range(1, len(parts), 3)}, "grid summary: " + summary


def _read_tree(d):
    return {str(p.relative_to(d)): p.read_bytes() for p in sorted(d.rglob("*")) if p.is_file()}


@pytest.mark.parametrize("ranked", [False, True])
def test_classify_grid_files_equal_the_single_calls(trained, tmp_path, monkeypatch, capfd, ranked):
    root, model_files, seq_files = trained
    monkeypatch.setenv("ECOZ2_VQ_GPUS", "1")
    points = _points(model_files, seq_files)
    assert len(points) == 9 and all(4 <= len(ms) <= 6 for ms, _ss in points.values())
    singles = _single_calls(points, tmp_path / "one", ranked, capfd)
    text = _grid_call(model_files, seq_files, tmp_path / "all", ranked, capfd)
    slices, summary = _split(text)
    assert list(slices) == list(points)  # N ascending, then M ascending
    for pt in points:
        assert slices[pt] == singles[pt], pt
    one, grid = _read_tree(tmp_path / "one"), _read_tree(tmp_path / "all")
    assert set(grid) == set(one) | {"summary.csv"}
    for k in one:
        assert one[k] == grid[k], k
    rows = grid["summary.csv"].decode().splitlines()
    assert rows[0] == "N,M,models,sequences,accuracy,avg_accuracy" and len(rows) == 1 + len(points)
    lines = summary.splitlines()
    assert lines[0] == f"grid summary: {len(points)} point(s)" and lines[-1] == "@/summary.csv saved"
    for row, line, (pt, (ms, ss)) in zip(rows[1:], lines[1:], points.items()):
        N, M, n_models, n_seqs, acc, avg = row.split(",")
        assert (int(N), int(M), int(n_models)) == (*pt, len(ms))
        rep = singles[pt]
        total = re.search(r"^\s+TOTAL\s+([\d.]+)%\s+(\d+)", rep, re.M)
        avg_rep = re.search(r"^  avg_accuracy\s+([\d.]+)%", rep, re.M)
        assert int(n_seqs) == int(total.group(2)) == len(ss)
        assert f"{float(acc):.2f}" == total.group(1) and f"{float(avg):.2f}" == avg_rep.group(1)
        assert line.split() == [f"N={pt[0]}", f"M={pt[1]}", f"models={len(ms)}", f"sequences={n_seqs}", f"accuracy={float(acc):.2f}",
                                f"avg_accuracy={float(avg):.2f}"]


def test_classify_grid_invariant_to_workers(trained, tmp_path, monkeypatch, capfd):
    root, model_files, seq_files = trained
    runs = []
    for gpus in ("1", "3"):
        monkeypatch.setenv("ECOZ2_VQ_GPUS", gpus)
        out = tmp_path / f"g{gpus}"
        runs.append((_grid_call(model_files, seq_files, out, True, capfd), _read_tree(out)))
    assert runs[0] == runs[1] and len(runs[0][1]) == 10


# ---- CLI -----------------------------------------------------------------------------------------------------------------
def test_classify_grid_cli_equals_the_library_call(tmp_path, capfd):
    env = dict(os.environ, NO_COLOR="1", ECOZ2_VQ_QUIET="1")
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_GPUS", "ECOZ2_HMM_SCORE_PACK"):
        env.pop(k, None)
    rng = np.random.default_rng(4)
    rows = ["tt,class,selection"]
    for c, cls in enumerate(["C00", "C01", "C02"]):
        for k in range(7):
            rows.append(f"{'TRAIN' if k < 5 else 'TEST'},{cls},{k:05d}")
            for M in (16, 33):
                s = np.clip((np.linspace(0, M - 1, 30) + 4 * c + rng.normal(0, 3, 30)).round(), 0, M - 1).astype(np.uint16)
                p = tmp_path / "data" / "sequences" / f"M{M}" / cls / f"{k:05d}.seq"
                p.parent.mkdir(parents=True, exist_ok=True)
                e.formats.write_seq(str(p), cls, M, s)
    (tmp_path / "tt.csv").write_text("\n".join(rows) + "\n")

    def run(*args):
        r = subprocess.run([EXE, "hmm", *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout

    run("learn", "--grid", "-N", "3,6", "-M", "16,33", "-s", "7", "-I", "3", "--sequences", "tt.csv")
    out = run("classify", "--grid", "-r", "--models", "data/hmms", "--tt", "TEST", "-M", "33,16", "-c", "cli/c12n", "--summary",
              "cli/summary.csv", "--sequences", "tt.csv")
    head = out.split("\n")
    assert head[0].startswith("ECOZ2 C version")
    assert head[1:4] == ["number of HMM models: 12  number of sequences: 12", "grid points: 4", "show_ranked = true"]
    # the library call on the lists the CLI resolves: models in resolve order, the TEST rows of M = 16, then of M = 33
    models = sorted(str(p.relative_to(tmp_path)) for p in (tmp_path / "data" / "hmms").rglob("*.hmm"))
    seqs = [f"data/sequences/M{M}/{cls}/{k:05d}.seq" for M in (16, 33) for cls in ("C00", "C01", "C02") for k in (5, 6)]
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        capfd.readouterr()
        e.hmm.hmm_classify_grid(models, seqs, True, "lib/c12n", "lib/summary.csv")
        text = capfd.readouterr().out
    finally:
        os.chdir(cwd)
    assert "\n".join(head[4:]).replace("cli/", "lib/") == text
    assert text.count("grid point: ") == 4 and "grid summary: 4 point(s)" in text
    cli, lib = _read_tree(tmp_path / "cli"), _read_tree(tmp_path / "lib")
    assert len(cli) == 5 and cli == lib
