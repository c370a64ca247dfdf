"""The batched HMM trainer (train_grid_batch: k_hmm_fb_grid, launch_fb, k_hmm_reestimate_grid, k_hmm_adjustb_grid;
DESIGN.md 4.8.3) at the launch shapes small corpora never reach: 2048 capped workgroups whose waves take two and three
sequences, a blocks table with several launches that shrinks as models stop, unsorted / nested / gapped sequence ranges,
one xi scratch shared by several N > 64, and more models than grid.y holds.  One e.hmm.train_grid call per case of
tests/hmm_learn_grid_cases.py; every model's pi, A, B and measure per iteration must equal the oracle's (H.learn on the
model's slice, empty sequences included) on their 64 bits.  test_hmm_learn_grid_cases_cpu.py shows, without a GPU, that
each case reaches the shape it names and that the oracle's bits move when the shape is cut short."""
import numpy as np
import pytest

import ecoz2rs_amd as e
from tests import hmm_learn_grid_cases as G
from tests import oracle_lib
from tests.test_gpu_hmm_learn_classes import _batched, _single_loop

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    return oracle_lib.load_hmm()


def _train_grid(case, key="seqs"):
    return e.hmm.train_grid(case["models"], case[key], case["ranges"], case["eps"], case["val_auto"], case["maxit"])


def _assert_oracle(got, want, what=""):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert G.same_bits(g, w), (what, k, g[3], w[3])


def _assert_single_training(case, got, key):
    """the models whose slice holds an empty sequence, against e2vq_hmm_train on that slice as it is -> how many"""
    n = 0
    for k, m in enumerate(case["models"]):
        seqs = G.slice_of(case, k, key)
        if all(len(s) for s in seqs):
            continue
        one = e.hmm.train(*m, seqs, case["eps"], case["val_auto"], case["maxit"])
        assert G.same_bits(got[k], one), k
        n += 1
    return n


def test_persistent_mid(H):
    """2048 capped workgroups from s_lo = 7, waves of two and three turns with every kind of bad sequence at each turn,
    a launch per N from its own offset of the blocks table, the second E-step on re-estimated parameters"""
    case = G.reference(H, "persistent_mid")
    got = _train_grid(case, "grid_seqs")
    _assert_oracle(got, case["want"], "grid")
    assert _assert_single_training(case, got, "grid_seqs") == 3


@pytest.mark.parametrize("name", ["persistent_mid", "big_n_scratch"])
def test_through_train_classes(H, name):
    """the same batch through e2vq_hmm_train_classes, which admits symbols >= M: the 'range' sequences as built (the
    models of persistent_mid that share N and M together, its N = 64 model, and each N of big_n_scratch)"""
    case = G.reference(H, name)
    for group in case["classes_groups"]:
        got = e.hmm.train_classes([case["models"][k] for k in group], [G.slice_of(case, k) for k in group], case["eps"],
                                  case["val_auto"], case["maxit"])
        _assert_oracle(got, [case["want_as_built"][k] for k in group], group)


def test_blocks_mix(H, monkeypatch):
    """workgroup counts 1, 1, 2, 9 and 2048 at three N; models leave the blocks table at different iterations, a
    2048-workgroup one before and after one-workgroup ones of its N.  The batch budget changes no bit."""
    case = G.reference(H, "blocks_mix")
    monkeypatch.delenv("ECOZ2_HMM_LEARN_BATCH_BYTES", raising=False)
    got = _train_grid(case)
    _assert_oracle(got, case["want"], "one batch")
    assert {len(g[3]) for g in got} == {2, 3, 4}
    for budget in ("1", "3000000"):  # every model a batch of its own; the small ones a few per batch
        monkeypatch.setenv("ECOZ2_HMM_LEARN_BATCH_BYTES", budget)
        _assert_oracle(_train_grid(case), case["want"], budget)


def test_ranges(H):
    """ranges given unsorted, one nested, one twice at different N, two gaps nobody trains on (one of them holding a
    symbol above every M), M differing between the runs"""
    case = G.reference(H, "ranges")
    _assert_oracle(_train_grid(case), case["want"])


def test_big_n_scratch(H):
    """N = 65, 141, 142 and 200 in one call, 70 sequences each on 64 persistent workgroups: one scratch sized for N = 200
    serves k_hmm_fb_wg<false> at 142 and at 200, and bad sequences sit at a workgroup's second turn"""
    case = G.reference(H, "big_n_scratch")
    got = _train_grid(case, "grid_seqs")
    _assert_oracle(got, case["want"])
    assert _assert_single_training(case, got, "grid_seqs") == 4


def test_many_models(H):
    """65 535 + 3 models of N = 1: the M-step's second grid.y launch holds the last three"""
    case = G.many_reference(H)
    models, ranges = G.many_models_of(case)
    got = e.hmm.train_grid(models, case["seqs"], ranges, case["eps"], case["val_auto"], case["maxit"])
    assert len(got) == G.MANY_K
    pair = np.array([G.many_pair_of(k) for k in range(G.MANY_K)])
    assert all(len(g[3]) == 2 for g in got)
    for i, name in enumerate(("pi", "A", "B", "hist")):
        have = G.bits(np.stack([np.asarray(g[i], dtype=np.float64).ravel() for g in got]))
        want = G.bits(np.stack([np.asarray(w[i], dtype=np.float64).ravel() for w in case["want"]]))[pair]
        wrong = np.flatnonzero((have != want).any(axis=1))
        assert wrong.size == 0, (name, wrong[:10].tolist(), wrong.size)


# ---- the skipped count of the file path ------------------------------------------------------------------------------
def _corpus_with_empty_files(root):
    """4 classes x 10 files at M = 16, interleaved; classes K1 and K3 hold empty sequences (T = 0), which every E-step
    skips and the `it=` lines of the training report"""
    rng = np.random.default_rng(77)
    files = []
    for q in range(10):
        for c in range(4):
            T = 0 if (c, q) in ((1, 0), (1, 6), (3, 9)) else int(rng.integers(10, 30))
            s = np.clip((np.linspace(0, 15, T) + 3 * c + rng.normal(0, 2, T)).round(), 0, 15).astype(np.uint16)
            p = root / "seqs" / f"K{c}" / f"{q:03d}.seq"
            p.parent.mkdir(parents=True, exist_ok=True)
            e.formats.write_seq(str(p), f"K{c}", 16, s)
            files.append(str(p))
    return files


def test_learn_classes_files_report_skipped_sequences(tmp_path, monkeypatch, capfd):
    """`hmm learn --all-classes` on a corpus with skipped sequences: stdout (the skipped count of every iteration), .hmm
    and .csv equal the loop of seeded ecoz2_hmm_learn calls"""
    monkeypatch.delenv("ECOZ2_VQ_QUIET", raising=False)
    monkeypatch.setenv("ECOZ2_VQ_GPUS", "1")
    files = _corpus_with_empty_files(tmp_path)
    assert len(files) == 40
    tree1, seen1, text1, K, _after1 = _single_loop(files, tmp_path / "one", monkeypatch, capfd, 5, 3, 4321, 1e-5, 0.3, 3)
    tree2, seen2, text2, _after2 = _batched(files, tmp_path / "all", monkeypatch, capfd, 5, 3, 4321, 1e-5, 0.3, 3)
    assert K == 4 and len(tree1) == 8 and tree1 == tree2 and seen1 == seen2
    assert text2.replace(str(tmp_path / "all"), "@") == text1.replace(str(tmp_path / "one"), "@")
    esteps = {c: len(v.splitlines()) - 2 for c in ("K1", "K3") for k, v in tree2.items() if k.endswith(f"{c}.csv")}
    assert set(esteps) == {"K1", "K3"} and min(esteps.values()) >= 2
    assert text2.count("(2 sequence(s) the model cannot emit were skipped)") == esteps["K1"]  # every E-step of class K1
    assert text2.count("(1 sequence(s) the model cannot emit were skipped)") == esteps["K3"]
    assert text2.count("were skipped") == esteps["K1"] + esteps["K3"]
