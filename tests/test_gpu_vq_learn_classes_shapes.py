"""`vq learn --all-classes` at the shapes the batched kernels can take: every order class of the MFMA
sweep (trailing coefficient counts 1 .. 4, the last narrow and the first wide orders, the spilling NC = 41), the three
accumulate modes, block tables with more than one block per wave and a `per` that changes within a level, codebooks
whose level record sums more than one chunk, classes of very different magnitudes, failed cells, the refusals found on
the device, orders below the MFMA sweep and hundreds of small classes.  Each class must be, bit for bit, the session
ladder of its frames alone (and the oracle where T x M is small); each test asserts from its outputs that the shape it
aims at was reached."""
import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import vq
from tests import oracle_lib
from tests.vq_classes_common import EPS, _batched, _bits, _class_frames, _prd_corpus, _same_levels, _session_ladder, _single_loop

pytestmark = pytest.mark.gpu
LDS_BYTES = 163840  # E2VQ_LDS_BYTES (vq_device.h)


# ---- the host rules, restated ------------------------------------------------------------------------------------------
def _row_stride(NC):
    return (2 * NC + 5 + 7) & ~7


def _hyb_cells(NC):
    """mfma_hyb_cells (vq_accum.h)"""
    return ((LDS_BYTES - 10240 - 8 * 16 * (2 * NC + 5 + 3) * 4) // (_row_stride(NC) * 8)) & ~7


def _mode(NC, M):
    """pass_classes_mode (vq_device.hip): the accumulate mode of the batched sweep at codebook size M"""
    if 41 < NC <= 81:
        return 2
    if M * _row_stride(NC) * 8 + 8 * 16 * (2 * NC + 5 + 3) * 4 + 2048 <= LDS_BYTES and M <= 128:
        return 1
    if M <= 4 * _hyb_cells(NC):
        return 5
    return 2


def _per(blocks):
    """the blocks of one table entry (train_batch in vq_classes.cpp): a multiple of the 8 waves, the table aiming at the 256
    workgroups of the single-set launch"""
    return max(8, (blocks + 255) // 256 + 7) // 8 * 8


def _schedule(sizes, ladders):
    """train_batch's table, rebuilt from the level records: class k is active in pass p of level l iff its passes there
    exceed p.  -> per level, per pass: (active classes, per, [(class, blocks) per entry])"""
    nb = [(T + 63) // 64 for T in sizes]
    out = []
    for l in range(len(ladders[0])):
        passes = [lv[l].passes for lv in ladders]
        lvl = []
        for p in range(max(passes)):
            act = [k for k in range(len(sizes)) if passes[k] > p]
            per = _per(sum(nb[k] for k in act))
            lvl.append((act, per, [(k, min(per, nb[k] - b)) for k in act for b in range(0, nb[k], per)]))
        out.append(lvl)
    return out


# ---- checks ------------------------------------------------------------------------------------------------------------
def _check_sessions(frames, P, max_M, got):
    assert len(got) == len(frames)
    for k, f in enumerate(frames):
        refl, levels = _session_ladder(f, P, max_M)
        cb, lv = got[k]
        assert np.array_equal(_bits(cb), _bits(refl)), (P, k)
        _same_levels(lv, levels)


def _check_oracle(frames, max_M, got):
    oracle = oracle_lib.load()
    for k, f in enumerate(frames):
        rc, lv_o, _cbs = oracle.learn(f, EPS, max_M)
        assert rc == 0
        cb, lv = got[k]
        assert [(l.M, l.passes, l.empty_cells) for l in lv] == [(l["M"], l["passes"], l["empty"]) for l in lv_o], k
        assert np.array_equal(_bits(cb), _bits(lv_o[-1]["reflections"])), k
        assert _bits([[l.DD, l.avg_distortion, l.sigma, l.inertia] for l in lv]).tolist() == \
            _bits([[l["DD"], l["avg"], l["sigma"], l["inertia"]] for l in lv_o]).tolist(), k


def _modes(P, got):
    return {_mode(P + 1, l.M) for l in got[0][1]}


# ---- 1. every order class of the sweep ---------------------------------------------------------------------------------
ORDERS = [4, 5, 6, 7, 8, 11, 15, 20, 31, 35, 39, 40, 41, 42, 47, 63, 64, 65, 79, 80]
ORACLE_ORDERS = {4, 7, 40, 41, 80}


def test_order_list_covers_every_tail_and_boundary():
    """REM = NC - 4 (ceil(NC / 4) - 1) = 1 .. 4 at narrow and at wide orders; NC = 41 (the spilling mode 1), 42, 43, 64, 65,
    81"""
    rem = lambda nc: nc - 4 * ((nc + 3) // 4 - 1)
    for wide in (False, True):
        assert {rem(P + 1) for P in ORDERS if (P + 1 > 41) == wide} == {1, 2, 3, 4}
    assert {41, 42, 43, 64, 65, 81} <= {P + 1 for P in ORDERS}


@pytest.mark.parametrize("P", ORDERS)
def test_orders_equal_session_ladders(P):
    sizes, max_M = [1, 65, 700, 3000], 256
    frames = _class_frames(P, sizes, seed=60 + P)
    got = vq.train_codebooks(frames, P, EPS, max_M)
    assert _modes(P, got) == ({2} if P + 1 > 41 else {1, 5})
    _check_sessions(frames, P, max_M, got)
    if P in ORACLE_ORDERS:
        _check_oracle(frames, max_M, got)


@pytest.mark.parametrize("P,max_M", [(5, 4096), (15, 2048), (40, 1024)])
def test_narrow_orders_reach_mode_2(P, max_M):
    """the first codebook size past the hybrid table at a narrow order: the global-atomic accumulate of mode 2"""
    frames = _class_frames(P, [3000, 9000], seed=80 + P)
    got = vq.train_codebooks(frames, P, EPS, max_M)
    assert _mode(P + 1, max_M) == 2 and _mode(P + 1, max_M // 2) == 5
    assert _modes(P, got) == {1, 5, 2}
    _check_sessions(frames, P, max_M, got)


# ---- 2. orders below the MFMA sweep ------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 3])
def test_tiny_orders_on_arrays(P):
    sizes, max_M = [1, 65, 700, 3000], 256
    frames = _class_frames(P, sizes, seed=90 + P)
    got = vq.train_codebooks(frames, P, EPS, max_M)
    assert [l.M for l in got[3][1]] == [2, 4, 8, 16, 32, 64, 128, 256]
    _check_sessions(frames, P, max_M, got)
    _check_oracle(frames, max_M, got)


@pytest.mark.parametrize("P", [1, 2, 3])
def test_tiny_orders_on_files_equal_the_single_loop(tmp_path, monkeypatch, capfd, P):
    monkeypatch.delenv("ECOZ2_VQ_QUIET", raising=False)
    monkeypatch.setenv("ECOZ2_VQ_GPUS", "1")
    monkeypatch.setenv("ECOZ2_VQ_MAX_CODEBOOK_SIZE", "256")
    sizes = [5, 300, 2000]
    files = _prd_corpus(tmp_path, P, sizes, seed=70 + P)
    tree1, seen1, text1, K = _single_loop(files, P, tmp_path / "one", monkeypatch, capfd)
    tree2, seen2, text2 = _batched(files, P, tmp_path / "all", monkeypatch, capfd)
    assert K == 3 and len(tree1) == K * 9
    assert tree1 == tree2 and seen1 == seen2
    assert text2.replace(str(tmp_path / "all"), "@") == text1.replace(str(tmp_path / "one"), "@")
    # ... and the codebooks and callbacks are the oracle's
    oracle = oracle_lib.load()
    by_class = {}
    for f in files:
        name, _p, part = e.formats.read_prd(f)
        by_class.setdefault(name, []).append(part)
    cbs = []
    for name in sorted(by_class, key=lambda s: s.encode()):
        rc, lv_o, cbs_o = oracle.learn(np.concatenate(by_class[name]), EPS, 256)
        assert rc == 0
        for l in lv_o:
            _n, _p, cb = e.formats.read_cbook(str(tmp_path / "all" / "data" / "codebooks" / name / f"eps_0.05_M_{l['M']:04d}.cbook"))
            assert np.array_equal(_bits(cb), _bits(l["reflections"])), (name, l["M"])
        cbs += cbs_o
    assert seen2 == cbs


# ---- 3. block tables: several blocks per wave, `per` changing within a level --------------------------------------------
@pytest.mark.parametrize("P", [36, 48])
def test_block_table_granularity(P):
    sizes, max_M = [100037, 40011, 2005], 256
    frames = _class_frames(P, sizes, seed=11)
    got = vq.train_codebooks(frames, P, EPS, max_M)
    sched = _schedule(sizes, [lv for _cb, lv in got])
    # some pass swept tables of 16 or more blocks per entry (two or more blocks per wave, four or more half blocks at wide
    # orders; mode 1 prefetches the next block) ...
    assert any(per >= 16 for lvl in sched for _a, per, _e in lvl), sched
    # ... a later pass of the same level a finer table, after classes ended the level ...
    assert any(lvl[q][1] < lvl[p][1] for lvl in sched for p in range(len(lvl)) for q in range(p + 1, len(lvl))), \
        [[per for _a, per, _e in lvl] for lvl in sched]
    # ... and a class ran over several entries, the last one short
    assert any(per >= 16 and sum(1 for k, _b in ent if k == c) > 1 and [b for k, b in ent if k == c][-1] < per
               for lvl in sched for _a, per, ent in lvl for c in range(len(sizes)))
    if P + 1 <= 41:
        assert _modes(P, got) == {1, 5}
    _check_sessions(frames, P, max_M, got)


# ---- 4. large codebooks ------------------------------------------------------------------------------------------------
def test_large_codebook_mode_2_two_record_chunks():
    """M = 8 192: the level record sums the within-cell terms in two chunks of 4 096"""
    P, max_M = 36, 8192
    frames = _class_frames(P, [23001, 29999], seed=21)
    got = vq.train_codebooks(frames, P, EPS, max_M)
    assert _mode(P + 1, max_M) == 2
    last = [lv[-1] for _cb, lv in got]
    assert all(l.M == 8192 for l in last)
    # fewer than 4 096 empty cells: some cell at index >= 4 096 is populated (the second chunk adds a term)
    assert any(l.empty_cells < 4096 for l in last), [l.empty_cells for l in last]
    _check_sessions(frames, P, max_M, got)


def test_large_codebook_mode_5_at_p4():
    P, max_M = 4, 4096
    frames = _class_frames(P, [20011, 26003, 24000], seed=22)
    got = vq.train_codebooks(frames, P, EPS, max_M)
    assert _mode(P + 1, 4096) == 5 and _mode(P + 1, 2048) == 5 and _hyb_cells(P + 1) == 1128
    _check_sessions(frames, P, max_M, got)


# ---- 5. per-class scalars ----------------------------------------------------------------------------------------------
def _scaled_classes(P):
    fs = [e.synth.synth_frames(51, 3, P, 0, 1500) * 2.0 ** -24,
          e.synth.synth_frames(52, 4, P, 0, 900),
          e.synth.synth_frames(53, 2, P, 0, 1300) * 2.0 ** 24,
          e.synth.synth_frames_kind(54, 1, 4, 0.05, P, 0, 2000)]
    return fs


@pytest.mark.parametrize("P", [12, 36, 48])
def test_per_class_scalars(P):
    """classes 2^48 apart in magnitude in one batch: each has its own fixed-point shifts (sc[k], l1max[k])"""
    frames, max_M = _scaled_classes(P), 256
    exps = [np.frexp(np.abs(f).max())[1] for f in frames]
    assert len(set(exps)) == len(frames), exps
    got = vq.train_codebooks(frames, P, EPS, max_M)
    _check_sessions(frames, P, max_M, got)
    if P == 36:
        _check_oracle(frames, max_M, got)


def test_classes_are_independent_of_neighbours_and_position():
    P, max_M = 36, 256
    frames = _scaled_classes(P)
    base = vq.train_codebooks(frames, P, EPS, max_M)
    K = len(frames)
    for k in range(K):
        others = [frames[i] for i in range(K) if i != k]
        for batch, at in (([frames[k]], 0), ([frames[k]] + others, 0), (others + [frames[k]], K - 1),
                          (others[::-1][:2] + [frames[k]], 2)):
            cb, lv = vq.train_codebooks(batch, P, EPS, max_M)[at]
            assert np.array_equal(_bits(cb), _bits(base[k][0])), (k, len(batch), at)
            _same_levels(lv, base[k][1])


# ---- 6. failed cells ---------------------------------------------------------------------------------------------------
def _with_failing_rows(P, n_good=1500, n_bad=60, seed=5):
    """good frames and rows r = [1, .9, -.9, 0 ...] (status 2 of the Levinson recursion for any sum of them): the global
    centroid is the good frames', the bad rows gather in a cell of their own, whose update fails"""
    rng = np.random.default_rng(seed)
    bad = np.zeros((n_bad, P + 1))
    bad[:, 0], bad[:, 1], bad[:, 2] = 1.0, 0.9, -0.9
    bad[:, :3] *= 1.0 + 1e-3 * rng.standard_normal((n_bad, 1))
    return np.concatenate([e.synth.synth_frames(9, 2, P, 0, n_good), bad]) if n_good else bad


@pytest.mark.parametrize("P", [36, 70])
def test_failed_cells_equal_the_session(P):
    """P = 36: k_cell_update<37> on the session side; P = 70: thread-per-cell kernels on both sides"""
    max_M = 128
    frames = _class_frames(P, [700, 2200], seed=3)
    frames.insert(1, _with_failing_rows(P))
    got = vq.train_codebooks(frames, P, EPS, max_M)
    assert any(l.failed_cells > 0 for l in got[1][1]), [l.failed_cells for l in got[1][1]]
    _check_sessions(frames, P, max_M, got)
    _check_oracle(frames, max_M, got)


# ---- 7. refusals found on the device ------------------------------------------------------------------------------------
def _bad_class(case, P):
    f = e.synth.synth_frames(61, 3, P, 0, 400)
    if case in ("nan", "inf", "-inf"):
        f[137, 5] = float(case)
    elif case == "zero":
        f[:] = 0.0
    else:  # every row fails the recursion: so does their sum, the global centroid
        f = _with_failing_rows(P, n_good=0, n_bad=400)
    return f


REASONS = {"nan": "contains NaN or infinite values", "inf": "contains NaN or infinite values",
           "-inf": "contains NaN or infinite values", "zero": "is all zeros",
           "levinson": "Levinson recursion failed on the global centroid"}


@pytest.mark.parametrize("P", [12, 48])
def test_device_refusals_on_arrays(P):
    max_M = 64
    good = _class_frames(P, [300, 1000, 64], seed=12)
    base = vq.train_codebooks(good, P, EPS, max_M)
    _check_sessions(good, P, max_M, base)
    for case, reason in REASONS.items():
        batch = good[:1] + [_bad_class(case, P)] + good[1:]
        with pytest.raises(e.Ecoz2Error) as ex:
            vq.train_codebooks(batch, P, EPS, max_M)
        assert "class 'class 1': " in str(ex.value) and reason in str(ex.value), (case, str(ex.value))
        # nothing of the failed call is left on the device
        again = vq.train_codebooks(good, P, EPS, max_M)
        for (a, la), (b, lb) in zip(base, again):
            assert np.array_equal(_bits(a), _bits(b)), case
            _same_levels(la, lb)


@pytest.mark.parametrize("gpus", ["1", "2"])
def test_device_refusals_on_files_write_nothing(tmp_path, monkeypatch, capfd, gpus):
    P = 36
    monkeypatch.setenv("ECOZ2_VQ_QUIET", "1")
    monkeypatch.setenv("ECOZ2_VQ_GPUS", gpus)
    monkeypatch.setenv("ECOZ2_VQ_MAX_CODEBOOK_SIZE", "64")
    files = _prd_corpus(tmp_path, P, [300, 1000, 64, 700], seed=13)
    base, seen_base, _t = _batched(files, P, tmp_path / "base", monkeypatch, capfd)
    assert len(base) == 4 * 7
    for i, (case, reason) in enumerate(REASONS.items()):
        bad = tmp_path / "bad" / case / "00000.prd"
        bad.parent.mkdir(parents=True, exist_ok=True)
        e.formats.write_prd(str(bad), "V02x", _bad_class(case, P))  # (between V02 and V03: a middle class)
        out = tmp_path / f"out{i}"
        with pytest.raises(e.Ecoz2Error) as ex:
            _batched(files + [str(bad)], P, out, monkeypatch, capfd)
        assert "class 'V02x': " in str(ex.value) and reason in str(ex.value), (case, str(ex.value))
        assert not out.exists() or not any(p.is_file() for p in out.rglob("*")), case
        tree, seen, _t = _batched(files, P, tmp_path / f"good{i}", monkeypatch, capfd)
        assert tree == base and seen == seen_base, case


# ---- 8. many small classes ---------------------------------------------------------------------------------------------
def test_many_small_classes():
    P, max_M, K = 12, 64, 300
    sizes = [1 + k % 200 for k in range(K)]
    frames = _class_frames(P, sizes, seed=17)
    got = vq.train_codebooks(frames, P, EPS, max_M)
    sched = _schedule(sizes, [lv for _cb, lv in got])
    assert len(sched[0][0][0]) == K and len(sched[0][0][2]) >= K  # grid.y = 300 classes; an entry or more each
    # the active list shrinks over several passes of a level, not all at once
    assert any(len({len(a) for a, _per, _e in lvl}) >= 3 for lvl in sched), [[len(a) for a, _p, _e in lvl] for lvl in sched]
    _check_sessions(frames, P, max_M, got)
