"""`hmm scan` at the edges of its staging area, of its run table and of its launches, against the CPU oracle:
every entry of every result is compared on its raw bits with what tests/hmm_scan_cases.py's `reference` builds from
H.forward and H.log_prob on the window's symbols -- never with hmm.score, whose kernel k_hmm_scan's step body copies.  The
rows of SCAN_SHAPES (a window of exactly, one less and one more than the 8192 staged symbols; runs cut by the span rule; 1 to
64 rounds; more than 2^20 windows under k_hmm_scan_wg; hops up to 2^63 - 1), under the three settings of
ECOZ2_HMM_SCAN_PACK; and status 1 and status 2 at every position of a window, staged and read from global memory.  What each
row reaches is asserted in test_hmm_scan_cpu.py."""
import time

import numpy as np
import pytest

from ecoz2rs_amd import hmm

from . import hmm_scan_cases as cases
from . import oracle_lib

pytestmark = pytest.mark.gpu

MATRIX = ("mant", "exp2", "status", "log_prob")
TOP = ("best", "second", "best_log_prob", "second_log_prob")


@pytest.fixture(scope="module")
def H():
    return oracle_lib.load_hmm()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def _equal(got, ref, what, rows=slice(None)):
    assert np.array_equal(got["win_offs"], ref["win_offs"]), what
    for key in MATRIX + TOP:
        if key in got:
            a, b = _bits(got[key])[rows], _bits(ref[key])[rows]
            assert a.shape == b.shape and a.dtype == b.dtype, (key, what)
            bad = np.argwhere(a != b)
            assert len(bad) == 0, (key, what, len(bad), bad[:5].tolist())


def _scan(models, streams, L, hop, **kw):
    sym, offs = hmm._pack(streams)
    t = time.perf_counter()
    got = hmm.scan(models, sym, offs, L, hop, **kw)
    got["wall_s"] = time.perf_counter() - t
    return got


# ---- 1. every row ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pack", cases.PACKS)
@pytest.mark.parametrize("name", [n for n in cases.SCAN_SHAPES if n != "many_windows" and not n.startswith("huge_hop")])
def test_every_row_equals_the_oracle(H, name, pack, monkeypatch):
    models, streams, L, (hop,) = cases.scan_shape(name)
    ref = cases.shape_reference(H, name, hop)
    _set(monkeypatch, "ECOZ2_HMM_SCAN_ROUNDS", None)
    _set(monkeypatch, "ECOZ2_HMM_SCAN_PACK", pack)
    got = _scan(models, streams, L, hop)
    print(name, pack, "windows", len(ref["mant"]), "scan %.3f s" % got["wall_s"], "kernels %.3f ms" % hmm.scan_last_kernel_ms())
    assert (ref["status"] == 0).all() and set(MATRIX) <= set(got)
    _equal(got, ref, (name, pack))
    top = _scan(models, streams, L, hop, matrix=False)
    assert "mant" not in top
    _equal(top, ref, (name, pack, "matrix=False"))


def test_many_windows_reach_the_second_launch_of_the_workgroup_kernel(H, monkeypatch):
    models, streams, L, (hop,) = cases.scan_shape("many_windows")
    ref = cases.shape_reference(H, "many_windows", hop)
    _set(monkeypatch, "ECOZ2_HMM_SCAN_ROUNDS", None)
    _set(monkeypatch, "ECOZ2_HMM_SCAN_PACK", None)
    got = _scan(models, streams, L, hop)
    print("many_windows: scan %.3f s" % got["wall_s"], "kernels %.3f ms" % hmm.scan_last_kernel_ms())
    W = len(ref["mant"])
    assert W == cases.WG_WINDOWS_PER_LAUNCH + 4
    _equal(got, ref, "the last four windows (the second launch of k_hmm_scan_wg)", rows=slice(W - 4, W))
    _equal(got, ref, "many_windows")
    top = _scan(models, streams, L, hop, matrix=False)
    _equal(top, ref, "many_windows, matrix=False")


# ---- 2. the rounds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", [None, "0", "1", "3", "64", "1000"])
@pytest.mark.parametrize("name", ["rounds_N1", "rounds_N21_N64"])
def test_the_rounds_change_no_bit(H, name, rounds, monkeypatch):
    models, streams, L, (hop,) = cases.scan_shape(name)
    ref = cases.shape_reference(H, name, hop)
    _set(monkeypatch, "ECOZ2_HMM_SCAN_PACK", None)
    _set(monkeypatch, "ECOZ2_HMM_SCAN_ROUNDS", rounds)
    got = _scan(models, streams, L, hop)
    print(name, rounds, "scan %.3f s" % got["wall_s"], "kernels %.3f ms" % hmm.scan_last_kernel_ms())
    _equal(got, ref, (name, rounds))


# ---- 3. and 4. events at every position of a window, staged and not ---------------------------------------------------------
def _events(H, case, at, monkeypatch, packs):
    models, clean, dirty, L, hop = case
    ref_clean, ref_dirty = cases.reference(H, models, clean, L, hop), cases.reference(H, models, dirty, L, hop)
    hit = np.array([bool(h) for h in cases.hits([len(s) for s in dirty], L, hop, 1, at)])
    assert hit.any() and not hit.all() and (ref_dirty["status"][hit] != 0).all() and (ref_dirty["status"][~hit] == 0).all()
    _set(monkeypatch, "ECOZ2_HMM_SCAN_ROUNDS", None)
    for pack in packs:
        _set(monkeypatch, "ECOZ2_HMM_SCAN_PACK", pack)
        got_clean, got_dirty = _scan(models, clean, L, hop), _scan(models, dirty, L, hop)
        print(pack, "scan %.3f s + %.3f s" % (got_clean["wall_s"], got_dirty["wall_s"]))
        _equal(got_clean, ref_clean, (pack, "clean"))
        _equal(got_dirty, ref_dirty, (pack, "dirty"))
        for key in MATRIX + TOP:  # a window the event does not lie in carries the bits it has in the clean stream
            assert np.array_equal(_bits(got_dirty[key])[~hit], _bits(got_clean[key])[~hit]), (key, pack)
    return ref_dirty


@pytest.mark.parametrize("kind", cases.EVENT_KINDS)
def test_an_event_at_every_position_of_the_window(H, kind, monkeypatch):
    ref = _events(H, cases.events_case(kind), cases.EVENT_AT, monkeypatch, cases.PACKS)
    assert set(np.unique(ref["status"])) == {0, cases.EVENT_STATUS[kind]}


@pytest.mark.parametrize("kind", cases.EVENT_KINDS)
def test_an_event_in_windows_read_from_global_memory(H, kind, monkeypatch):
    ref = _events(H, cases.unstaged_events_case(kind), cases.UNSTAGED_EVENT_AT, monkeypatch, cases.PACKS)
    want = [cases.EVENT_STATUS[kind]] * 4 + [0] * 3 + [cases.EVENT_STATUS[kind]] + [0]
    assert (ref["status"] == np.array(want)[:, None]).all()


# ---- 5. hops up to 2^63 - 1 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pack", cases.PACKS)
@pytest.mark.parametrize("name", ["huge_hop_long", "huge_hop_short"])
def test_a_huge_hop_gives_what_any_hop_of_one_window_a_stream_gives(H, name, pack, monkeypatch):
    models, streams, L, hops = cases.scan_shape(name)
    _set(monkeypatch, "ECOZ2_HMM_SCAN_ROUNDS", None)
    _set(monkeypatch, "ECOZ2_HMM_SCAN_PACK", pack)
    got8 = _scan(models, streams, L, hops[0])
    assert hmm.scan_last_kernel_ms() > 0
    _equal(got8, cases.shape_reference(H, name, hops[0]), (name, pack, hops[0]))
    first = got8["win_offs"][:-1]  # the first window of every stream: all there is at the larger hops
    assert np.array_equal(np.diff(got8["win_offs"]), [1, 1, 1] if name == "huge_hop_long" else [1, 7, 1])
    for hop in hops[1:]:
        got = _scan(models, streams, L, hop)
        assert hmm.scan_last_kernel_ms() > 0, hop
        assert got["win_offs"].tolist() == [0, 1, 2, 3], hop
        _equal(got, cases.shape_reference(H, name, hop), (name, pack, hop))
        for key in MATRIX + TOP:
            assert np.array_equal(_bits(got[key]), _bits(got8[key])[first]), (key, name, pack, hop)
