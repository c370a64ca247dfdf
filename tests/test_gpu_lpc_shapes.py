"""GPU tests of the LPC kernels at every order and at the window, status and launch edges: each lane-per-frame
instantiation of E2VQ_LPC_NC_LIST in both modes and in the feature kernels, the block and generic kernels at the smallest
and largest orders and just off a lane order, frame lengths around each phase of the lane autocorrelation, what a row
that stops early leaves in pe, rc and a, frame counts around the 256-thread block and the 64-lane wave, the grid-stride
loop, the generic path's window limit, and a signal batch whose files end on and next to a wave boundary.

Every comparison is on the bits of float64 and the values of int32 against the numpy restatements (tests/lpc_restatement.py,
tests/lpc_features_restatement.py): the contract is equality, there is no tolerance here."""
import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import formats
from tests import lpc_features_restatement as F
from tests import lpc_restatement as R
from tests import lpc_wavs
from tests.test_gpu_lpc_features import _check, _hand_rows
from tests.test_lpc_cpu import GENERIC, LANE, frame_lengths, lpca_rows

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -(2 ** 31), 2 ** 31 - 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, ref, what):
    """Bit equality; where the restatement holds a NaN, a NaN (its payload is not part of the contract)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, what
    if ref.dtype == np.int32:
        assert got.dtype == np.int32 and np.array_equal(got, ref), what
        return
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    bad = np.argwhere((_bits(got) != _bits(ref)) & ~nan)
    assert len(bad) == 0, (what, "first (row, column) that differs:", bad[:1].tolist())


def _check_lpca(x, P, what):
    """lpca_batch against R.lpca on every row, failed rows included -> the statuses"""
    got = e.lpc.lpca_batch(x, P)
    ref = R.lpca(x, P)
    for name, g, r in zip(("status", "pe", "r", "rc", "a"), got, ref):
        _same(g, r, (name,) + what)
    return ref[0]


# ---- a. lpca_batch, windowed mode: every order, frame lengths around each phase of the autocorrelation ---------------
@pytest.mark.parametrize("P", LANE + GENERIC)
def test_lpca_batch_every_order_and_frame_length(P):
    """n = NC runs the first phase only (and its static predicate to the end), NC < n < 2 NC the tail without the main
    loop, n = 2 NC and 3 NC an empty tail.  Rows that stop early (status 1 and 2) are compared like the others."""
    for n in frame_lengths(P + 1):
        st = _check_lpca(lpca_rows(P, n), P, (P, n))
        assert set(st) == {0, 1, 2}, (P, n)


# ---- b. frame counts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [16, 13])
def test_lpca_batch_frame_counts(P):
    """1, 63, 64, 65 and 257 frames: one lane, a wave partly and just past the end, the second 256-thread block."""
    n = 2 * (P + 1) + 1
    rows = lpca_rows(P, n)
    rows = rows[np.random.default_rng(P).permutation(len(rows))]  # all three statuses among the first few
    for count in (1, 63, 64, 65, 257):
        st = _check_lpca(rows[:count], P, (P, count))
        assert count < 63 or set(st) == {0, 1, 2}, (P, count)


def test_lpca_batch_grid_stride_above_65536_frames():
    """65 536 + 3 rows at P = 2: the blocks of k_lpc_block that take a second frame reuse their LDS; the last three rows
    (a normal row, the zero row, one sample at the end) differ from each other and from the rows 65 536 before them."""
    P, n = 2, 5
    base = lpca_rows(P, n)
    rows = np.concatenate([base] * (65536 // len(base) + 1))[:65536]
    last = np.array([[0.3, -1.1, 0.7, 0.2, -0.4], [0.0] * 5, [0.0, 0.0, 0.0, 0.0, -2.5]])
    st = _check_lpca(np.concatenate([rows, last]), P, ("grid stride",))
    assert list(st[-3:]) == [0, 1, 0] and set(st) == {0, 1, 2}


# ---- c. analyze, signal mode: the window against NC --------------------------------------------------------------------
def _check_analyze(s, P, win, off, T):
    what = (P, win, off)
    frames, status = e.lpc.analyze(s, 1000, P=P, W=win, O=off)  # 1000 Hz: a window of W ms is W samples
    f_r, st_r = R.analyze(s, 1000, P=P, W=win, O=off)
    assert len(st_r) == T, what
    _same(status, st_r, ("status",) + what)
    _same(frames, f_r, ("frames",) + what)
    return st_r


def _windows(NC):
    return (2, NC - 1, NC, NC + 1, 2 * NC - 1, 2 * NC, 2 * NC + 1, 5 * NC)


@pytest.mark.parametrize("P", LANE + (13, 80))
def test_analyze_window_against_nc(P):
    """win <= P included: the lags beyond the window are zero sums on both paths, as in the restatement.  65 frames at an
    offset of one sample (a constant stretch gives status 1 among them) and one frame at an offset of half a window."""
    src = lpc_wavs.to_pcm(lpc_wavs.ar_source(100 + P, 10, 5 * 81 + 64, 0.6), 16)
    for win in _windows(P + 1):
        s = src[:win + 64].copy()
        s[10:10 + win + 5] = 7  # frames 10 .. 15 are constant: zero after mean removal
        st = _check_analyze(s, P, win, 1, 65)
        assert (st[10:16] == 1).all() and (st == 0).any(), (P, win)
        _check_analyze(src[40:40 + win], P, win, max(1, win // 2), 1)


@pytest.mark.parametrize("P", [16, 13])
def test_analyze_int32_extremes_side_by_side(P):
    NC = P + 1
    s = lpc_wavs.to_pcm(lpc_wavs.ar_source(7, 10, 5 * NC + 64, 0.6), 32)
    s[NC:NC + 4] = [INT32_MIN, INT32_MAX, INT32_MAX, INT32_MIN]
    for win in (NC - 1, 2 * NC + 1, 5 * NC):
        st = _check_analyze(s[:win + 64], P, win, 1, 65)
        assert (st == 0).all(), (P, win)


# ---- d. long windows -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_signal():
    return lpc_wavs.to_pcm(lpc_wavs.ar_source(31, 10, 7681 + 100, 0.6), 16)


def test_generic_path_at_its_window_limit(long_signal):
    st = _check_analyze(long_signal[:7680 + 100], 80, 7680, 100, 2)
    assert (st == 0).all()


def test_generic_path_refuses_past_its_window_limit(long_signal):
    with pytest.raises(e.Ecoz2Error, match="generic path, whose window limit is 7680 samples"):
        e.lpc.analyze(long_signal, 1000, P=80, W=7681, O=100)
    with pytest.raises(e.Ecoz2Error, match="generic path, whose frame limit is 7680 samples"):
        e.lpc.lpca_batch(np.ones((2, 7681)), 80)


def test_lane_path_has_no_window_limit(long_signal):
    st = _check_analyze(long_signal, 12, 7681, 100, 2)
    assert (st == 0).all()


# ---- e. ecoz2_lpc_signals: files that end on and next to a wave boundary before the window changes ---------------------
@pytest.mark.parametrize("P", [16, 13])
def test_lpc_signals_wave_boundaries(P, tmp_path, monkeypatch):
    """Sorted, the three files have 64, 1 and 63 frames at three window lengths: the frame table needs no padding after
    the first, 63 padding entries after the second and one after the third."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("ECOZ2_VQ_OUT_ROOT", raising=False)
    W, O = 10, 5
    files = {}
    for name, sr, T in (("a", 16000, 64), ("b", 22050, 1), ("c", 32000, 63)):
        win, off = W * sr // 1000, O * sr // 1000
        s = lpc_wavs.to_pcm(lpc_wavs.ar_source(40 + T, 10, win + (T - 1) * off, 0.6), 16)
        assert R.geometry(len(s), sr, W, O) == (win, off, T)
        lpc_wavs.write_wav(tmp_path / "signals" / "K" / (name + ".wav"), s, sr, 16)
        files[name] = (s, sr)
    e.lpc.lpc_signals(P, W, O, 0, 0.0, [f"signals/K/{name}.wav" for name in sorted(files)], mintrpt=1e9)
    for name, (s, sr) in files.items():
        f_r, st_r = R.analyze(s, sr, P=P, W=W, O=O)
        ref = tmp_path / "ref.prd"
        formats.write_prd(str(ref), "K", f_r[st_r == 0])
        got = tmp_path / "data" / "predictors" / "K" / (name + ".prd")
        assert got.read_bytes() == ref.read_bytes(), (P, name)


# ---- f. features at the orders no other test runs ----------------------------------------------------------------------
@pytest.mark.parametrize("P", [16, 20, 24, 28, 32, 1, 2, 13, 79])
def test_features_at_every_other_order(P):
    hand = _hand_rows(P)
    if P == 1:  # no middle k: r = [1, 3] gives akk = -3 and pe = 1 - 9 at the only step
        hand = np.array([[0.0, 0.5], [0.0, 0.0], [1.0, 3.0], [1.0, 0.9]])
    r = np.concatenate([e.synth.synth_frames(7, 4, P, 0, 100), hand])
    for q in sorted({P + 1, e.lpc.MAX_Q} | ({48} if 48 > P else set())):
        ref = F.features(r, q)
        assert set(ref["status"]) == {0, 1, 2}, (P, q)
        _check(e.lpc.features(r, q=q), ref)
    ref = F.features(r, P + 1)
    _check(e.lpc.features(r, q=P + 1, want=("c",)), ref)
    _check(e.lpc.features(r, want=("a",)), ref)
    _check(e.lpc.features(r, want=("status", "rc")), ref)
