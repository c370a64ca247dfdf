"""`vq learn --all-classes` on the GPU: every class's codebook ladder trained in one batched training
must be the single-class ladder's, bit for bit -- on arrays (e2vq_vq_train_classes against per-class VqSession ladders
and the oracle), on files (e2vq_vq_learn_classes against a loop of ecoz2_vq_learn calls: .cbook, .rpt, stdout,
callbacks), for any ECOZ2_VQ_GPUS, batch budget and solo threshold, through the CLI, and for an order without an MFMA
sweep (P = 100, the single-class route inside the call)."""
import os
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import vq
from tests import oracle_lib
from tests.vq_classes_common import (EPS, _batched, _bits, _class_frames, _prd_corpus, _read_tree, _same_levels,
                                     _session_ladder, _single_loop)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 63, 65, 700, 4000, 20000]  # K = 6 classes, from one frame to a few tens of thousands


@pytest.mark.parametrize("P", [12, 36, 48])
@pytest.mark.parametrize("max_M", [256, 2048])
def test_train_codebooks_equals_session_ladders(P, max_M):
    frames = _class_frames(P, SIZES)
    got = vq.train_codebooks(frames, P, EPS, max_M)
    assert len(got) == len(SIZES)
    passes = []
    for k, f in enumerate(frames):
        refl, levels = _session_ladder(f, P, max_M)
        cb, lv = got[k]
        assert cb.shape == (max_M, P + 1)
        assert np.array_equal(_bits(cb), _bits(refl)), k
        _same_levels(lv, levels)
        passes.append([l.passes for l in lv])
    # the classes end levels after different numbers of passes: the inactive-class path ran
    assert any(len({p[i] for p in passes}) > 1 for i in range(len(passes[0]))), passes
    # small classes at large M: empty cells
    assert got[0][1][-1].empty_cells == max_M - 1


def test_train_codebooks_equals_the_oracle():
    P, max_M = 36, 256
    frames = _class_frames(P, SIZES[:5])
    got = vq.train_codebooks(frames, P, EPS, max_M)
    oracle = oracle_lib.load()
    for k, f in enumerate(frames):
        rc, lv_o, _cbs = oracle.learn(f, EPS, max_M)
        assert rc == 0
        cb, lv = got[k]
        assert [l.passes for l in lv] == [l["passes"] for l in lv_o], k
        assert np.array_equal(_bits(cb), _bits(lv_o[-1]["reflections"])), k
        assert [(l.M, l.empty_cells) for l in lv] == [(l["M"], l["empty"]) for l in lv_o]
        assert _bits([l.avg_distortion for l in lv]).tolist() == _bits([l["avg"] for l in lv_o]).tolist()


@pytest.mark.parametrize("P", [36, 48])
def test_block_boundaries(P):
    """T_k = 1, 63, 64, 65 (and two blocks, two blocks and one): each class's last block ends at its own T_k"""
    sizes = [1, 63, 64, 65, 128, 129]
    frames = _class_frames(P, sizes, seed=31)
    got = vq.train_codebooks(frames, P, EPS, 64)
    for k, f in enumerate(frames):
        refl, levels = _session_ladder(f, P, 64)
        assert np.array_equal(_bits(got[k][0]), _bits(refl)), sizes[k]
        _same_levels(got[k][1], levels)


def test_train_codebooks_routes_are_invisible(monkeypatch):
    P, max_M = 36, 512
    frames = _class_frames(P, SIZES)
    base = vq.train_codebooks(frames, P, EPS, max_M)
    for env in ({"ECOZ2_VQ_LEARN_BATCH_BYTES": "1"}, {"ECOZ2_VQ_LEARN_CLASSES_SOLO_FRAMES": "3000"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        other = vq.train_codebooks(frames, P, EPS, max_M)
        for k in env:
            monkeypatch.delenv(k)
        for (a, la), (b, lb) in zip(base, other):
            assert np.array_equal(_bits(a), _bits(b))
            _same_levels(la, lb)


# ---- files ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,max_M", [(36, 1024), (12, 256)])
def test_learn_classes_files_equal_the_single_loop(tmp_path, monkeypatch, capfd, P, max_M):
    monkeypatch.delenv("ECOZ2_VQ_QUIET", raising=False)
    monkeypatch.setenv("ECOZ2_VQ_GPUS", "1")
    monkeypatch.setenv("ECOZ2_VQ_MAX_CODEBOOK_SIZE", str(max_M))
    files = _prd_corpus(tmp_path, P, SIZES)
    tree1, seen1, text1, K = _single_loop(files, P, tmp_path / "one", monkeypatch, capfd)
    tree2, seen2, text2 = _batched(files, P, tmp_path / "all", monkeypatch, capfd)
    levels = max_M.bit_length() - 1
    assert K == len(SIZES) and len(tree1) == K * (levels + 1)
    assert tree1.keys() == tree2.keys()
    for k in tree1:
        assert tree1[k] == tree2[k], k
    assert seen2 == seen1 and len(seen1) == K * levels
    assert text2.replace(str(tmp_path / "all"), "@") == text1.replace(str(tmp_path / "one"), "@")
    assert text2.count("Codebook generation:") == K and "WARN: review_cells" in text2


def test_learn_classes_invariant_to_workers_batches_and_route(tmp_path, monkeypatch, capfd):
    monkeypatch.setenv("ECOZ2_VQ_QUIET", "1")
    monkeypatch.setenv("ECOZ2_VQ_MAX_CODEBOOK_SIZE", "512")
    P = 36
    files = _prd_corpus(tmp_path, P, SIZES, seed=6)
    runs = []
    cases = [dict(ECOZ2_VQ_GPUS="1"), dict(ECOZ2_VQ_GPUS="2"), dict(ECOZ2_VQ_GPUS="3"),
             dict(ECOZ2_VQ_GPUS="1", ECOZ2_VQ_LEARN_BATCH_BYTES="1"),
             dict(ECOZ2_VQ_GPUS="2", ECOZ2_VQ_LEARN_CLASSES_SOLO_FRAMES="3000")]
    for i, env in enumerate(cases):
        for k in ("ECOZ2_VQ_LEARN_BATCH_BYTES", "ECOZ2_VQ_LEARN_CLASSES_SOLO_FRAMES"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        tree, seen, text = _batched(files, P, tmp_path / f"r{i}", monkeypatch, capfd)
        runs.append((tree, seen, text.replace(str(tmp_path / f"r{i}"), "@")))
    assert len(runs[0][0]) == len(SIZES) * 10  # (M = 2 .. 512 and the report)
    for r in runs[1:]:
        assert r == runs[0]


def test_learn_classes_generic_order_takes_the_single_route(tmp_path, monkeypatch, capfd):
    """P = 100 has no MFMA sweep: every class trains through the session path inside the call, with the same output"""
    monkeypatch.delenv("ECOZ2_VQ_QUIET", raising=False)
    monkeypatch.setenv("ECOZ2_VQ_GPUS", "1")
    monkeypatch.setenv("ECOZ2_VQ_MAX_CODEBOOK_SIZE", "64")
    P = 100
    files = _prd_corpus(tmp_path, P, [5, 300, 900], seed=8)
    tree1, seen1, text1, K = _single_loop(files, P, tmp_path / "one", monkeypatch, capfd)
    tree2, seen2, text2 = _batched(files, P, tmp_path / "all", monkeypatch, capfd)
    assert K == 3 and tree1 == tree2 and seen1 == seen2
    assert text2.replace(str(tmp_path / "all"), "@") == text1.replace(str(tmp_path / "one"), "@")


def test_learn_classes_cli(tmp_path):
    exe = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
    env = dict(os.environ, ECOZ2_VQ_MAX_CODEBOOK_SIZE="256")
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_QUIET", "ECOZ2_VQ_LEARN_BATCH_BYTES", "ECOZ2_VQ_GPUS",
              "ECOZ2_VQ_LEARN_CLASSES_SOLO_FRAMES"):
        env.pop(k, None)
    P = 36
    classes = ["C00", "C01", "C02"]
    rows = ["tt,class,selection"]
    for c, cls in enumerate(classes):
        f = _class_frames(P, [40 * (c + 1) * 9], seed=40 + c)[0]
        for k, part in enumerate(np.array_split(f, 9)):
            p = tmp_path / "data" / "predictors" / cls / f"{k:05d}.prd"
            p.parent.mkdir(parents=True, exist_ok=True)
            e.formats.write_prd(str(p), cls, part)
            rows.append(f"{'TRAIN' if k < 6 else 'TEST'},{cls},{k:05d}")
    (tmp_path / "tt.csv").write_text("\n".join(rows) + "\n")

    def run(root, *args):
        r = subprocess.run([exe, *args], cwd=tmp_path, env=dict(env, ECOZ2_VQ_OUT_ROOT=str(tmp_path / root)),
                           capture_output=True, text=True, timeout=600)
        return r.returncode, r.stdout, r.stderr

    for cls in classes:
        rc, out, err = run("one", "vq", "learn", "-P", str(P), "--class-name", cls, "--predictors", "tt.csv")
        assert rc == 0 and "Codebook generation:" in out, (out, err)
    rc, out, err = run("all", "vq", "learn", "--all-classes", "-P", str(P), "--predictors", "tt.csv")
    assert rc == 0, err
    assert out.split("\n")[:2] == ["predictor files: 18", "classes: 3"], out
    assert out.count("Codebook generation:") == 3
    one, all_ = _read_tree(tmp_path / "one" / "data" / "codebooks"), _read_tree(tmp_path / "all" / "data" / "codebooks")
    assert len(one) == 3 * 9 and one == all_
    # directory inputs: the TRAIN and TEST files of every class
    for cls in classes:
        rc, out, err = run("dir1", "vq", "learn", "-P", str(P), "--class-name", cls, "--predictors", f"data/predictors/{cls}")
        assert rc == 0, err
    rc, out, err = run("dir2", "vq", "learn", "--all-classes", "-P", str(P), "--predictors", "data/predictors")
    assert rc == 0 and out.split("\n")[:2] == ["predictor files: 27", "classes: 3"], (out, err)
    assert _read_tree(tmp_path / "dir1") == _read_tree(tmp_path / "dir2")
