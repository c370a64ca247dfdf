"""The cases of tests/hmm_learn_grid_cases.py, on the oracle alone: each case reaches the launch shape it names (shown
from the host rules restated there: workgroup counts, turns per wave, the blocks table's offsets, the merged runs, the
grid.y split), each bad sequence sits at its intended turn and gets its intended oracle status, and the comparison of
test_gpu_hmm_learn_grid_shapes.py can bite: the oracle's trained bits change when the sequences of the later turns are
withheld, when a range reaches into its unused neighbours, when a model gets its neighbour's class."""
import numpy as np
import pytest

import ecoz2rs_amd as e
from tests import hmm_learn_grid_cases as G
from tests import oracle_lib


@pytest.fixture(scope="module")
def H():
    return oracle_lib.load_hmm()


STATUS = {"empty": 1, "range": 2, "emit": 1}


def _check_bad(H, case, k, slot):
    """the bad sequences of model k: each at the turn its index says, with the oracle's status for its kind under the
    initial model; every other sequence of its wave (workgroup) is used.  -> {turn: kinds met there}"""
    m, bad = case["models"][k], case["bad"][k]
    S = case["ranges"][k][1] - case["ranges"][k][0]
    met = {}
    for key in ("seqs", "grid_seqs"):
        seqs = G.slice_of(case, k, key)
        _acc, res = H.accumulate(*m, seqs)
        for i, kind in bad.items():
            want = STATUS[kind] if key == "seqs" else 1  # (a 'range' sequence is an 'emit' one in grid_seqs)
            assert res[i][0] == want, (k, i, kind, key)
            if kind == "empty":
                assert res[i] == (1, 0.5, 1) and len(seqs[i]) == 0
            mates = [j for j in range(S) if j != i and slot(j, S)[:-1] == slot(i, S)[:-1]]
            assert mates and all(res[j][0] == 0 for j in mates if j not in bad), (k, i)
            met.setdefault(slot(i, S)[-1], set()).add(kind)
        # what the counters of the E-step see: every sequence is used or skipped
        assert _acc[-2] + _acc[-1] == S and _acc[-1] >= len(bad)
    return met


def test_oracle_takes_empty_sequences(H):
    """H.learn on a slice with T = 0 sequences equals H.learn without them (an empty sequence adds nothing and counts as
    skipped), so the GPU tests give the oracle the slices as they are"""
    case = G.reference(H, "persistent_mid")
    for k in (1, 4):
        seqs = G.slice_of(case, k, "grid_seqs")
        kept = [s for s in seqs if len(s)]
        assert 0 < len(kept) < len(seqs)
        assert G.same_bits(case["want"][k], G.oracle_train(H, case, k, seqs=kept))


def test_persistent_mid_reaches_its_shape(H):
    case = G.reference(H, "persistent_mid")
    Ns = [len(m[0]) for m in case["models"]]
    Ss = [hi - lo for lo, hi in case["ranges"]]
    assert Ns == [5, 5, 5, 3, 64] and [m[2].shape[1] for m in case["models"]] == [8, 8, 12, 8, 8]
    assert Ss == [7, G.S_B, 13, G.S_B, G.S_D] and case["ranges"][1] == case["ranges"][3] and case["ranges"][1][0] == 7
    assert [G.fb_class_workgroups(S) for S in Ss] == [2, 2048, 4, 2048, 2048]
    turns_b, turns_c, turns_d = (G.wave_turns(S) for S in (G.S_B, 13, G.S_D))
    assert sorted(set(turns_b.values())) == [2, 3] and sum(t == 3 for t in turns_b.values()) == 37
    assert [turns_c[(3, w)] for w in range(4)] == [1, 0, 0, 0] and all(turns_c[(g, w)] == 1 for g in range(3) for w in range(4))
    assert sorted(set(turns_d.values())) == [1, 2] and sum(t == 2 for t in turns_d.values()) == 300
    # one launch per N, each from its own offset of the table; both iterations run every model (max_iterations = 2)
    rows, launches = G.blocks_table(Ns, Ss, range(5))
    assert launches == [(3, 0, 2048), (5, 2048, 2 + 2048 + 4), (64, 2048 + 2054, 2048)] and len(rows) == 6150
    assert rows[2048] == (0, 0, 2) and rows[2050] == (1, 0, 2048) and rows[-1] == (4, 2047, 2048)
    assert all(len(w[3]) == 2 for w in case["want"])
    for k in (1, 3):  # class b: every kind at the first, second and third turn of a wave that takes three
        met = _check_bad(H, case, k, G.wave_slot)
        assert met == {0: {"empty", "range", "emit"}, 1: {"empty", "range", "emit"}, 2: {"empty", "range", "emit"}}
        for i in G.BAD_B:
            if i % 8192 < 37:
                assert turns_b[G.wave_slot(i, G.S_B)[:2]] == 3
    assert _check_bad(H, case, 4, G.wave_slot) == {0: {"empty", "range", "emit"}, 1: {"empty", "range", "emit"}}
    assert max(len(s) for s in G.slice_of(case, 4)) <= 4 and max(len(s) for s in G.slice_of(case, 1)) <= 7
    # the second E-step runs on re-estimated parameters, and a 'range' sequence is not an 'emit' one there: epsilon
    # floors the unemittable column, so the two kinds part in the second measure
    for k in (1, 4):
        assert case["want"][k][3][0] == case["want_as_built"][k][3][0] and case["want"][k][3][1] != case["want_as_built"][k][3][1]


@pytest.mark.parametrize("k", [1, 3, 4])
def test_persistent_mid_later_turns_matter(H, k):
    """a wave that stopped after its first sequence would train on the first 8192 only: other bits"""
    case = G.reference(H, "persistent_mid")
    first = G.slice_of(case, k, "grid_seqs")[:8192]
    assert not G.same_bits(case["want"][k], G.oracle_train(H, case, k, seqs=first))
    if k != 4:  # and the third turn alone
        two = G.slice_of(case, k, "grid_seqs")[:2 * 8192]
        assert not G.same_bits(case["want"][k], G.oracle_train(H, case, k, seqs=two))


def test_grid_entry_refuses_the_range_kind(H):
    """why the grid call gets grid_seqs: a symbol >= M_k in model k's range is refused before the device"""
    case = G.reference(H, "persistent_mid")
    with pytest.raises(e._lib.Ecoz2Error, match="model 1: symbol 8 outside the codebook size 8"):
        e.hmm.train_grid(case["models"], case["seqs"], case["ranges"], case["eps"], case["val_auto"], case["maxit"])


def test_blocks_mix_reaches_its_shape(H):
    case = G.reference(H, "blocks_mix")
    Ns = [len(m[0]) for m in case["models"]]
    Ss = [hi - lo for lo, hi in case["ranges"]]
    assert sorted(set(zip(Ns, Ss))) == sorted((N, S) for N in G.MIX_NS for S in G.MIX_SIZES) and len(Ns) == 15
    wgs = {S: G.fb_class_workgroups(S) for S in G.MIX_SIZES}
    assert list(wgs.values()) == [1, 1, 2, 9, 2048]
    stops = {(N, S): len(w[3]) for N, S, w in zip(Ns, Ss, case["want"])}
    assert set(stops.values()) == {2, 3, 4}
    ones = [S for S in G.MIX_SIZES if wgs[S] == 1]
    assert any(stops[(N, 8193)] > stops[(N, S)] for N in G.MIX_NS for S in ones)  # a 2048-workgroup model outlives ...
    assert any(stops[(N, 8193)] < stops[(N, S)] for N in G.MIX_NS for S in ones)  # ... and is outlived by a one-workgroup one
    # so the table shrinks from both ends: the launches of each iteration, from the models the oracle says still run
    tables = [G.blocks_table(Ns, Ss, [k for k in range(15) if len(case["want"][k][3]) > it])[1] for it in range(4)]
    assert tables[0] == tables[1] and len({tuple(t) for t in tables[1:]}) == 3 and all(len(t) == 3 for t in tables)
    assert [at for _N, at, _n in tables[0]] == [0, 2061, 4122]


def test_ranges_reaches_its_shape(H):
    case = G.reference(H, "ranges")
    assert case["ranges"] == [(60, 100), (0, 10), (30, 31), (65, 90), (60, 100)] and len(case["seqs"]) == 100
    assert case["ranges"] != sorted(case["ranges"])
    runs, at = G.merged_runs(case["ranges"])
    assert runs == [(0, 10), (30, 31), (60, 100)] and at == [0, 10, 11]
    assert [G.local_index(case["ranges"], lo) for lo, _hi in case["ranges"]] == [11, 0, 10, 16, 11]
    used = {s for lo, hi in runs for s in range(lo, hi)}
    assert set(range(100)) - used == set(range(10, 30)) | set(range(31, 60)) and G.POISON not in used
    Ms = [m[2].shape[1] for m in case["models"]]
    assert len({Ms[0], Ms[1], Ms[2]}) == 3 and int(case["seqs"][G.POISON].max()) > max(Ms)
    assert len(case["models"][4][0]) != len(case["models"][0][0])
    for k, (lo, hi) in enumerate(case["ranges"]):
        assert max(int(s.max()) for s in case["seqs"][lo:hi]) < Ms[k]
    # a wrong run or a wrong local index hands a model other sequences: every sequence differs from every other one
    assert len({s.tobytes() for s in case["seqs"]}) == 100


@pytest.mark.parametrize("k,lo,hi", [(1, 0, 11), (2, 30, 32), (2, 29, 31), (0, 59, 100), (3, 65, 91), (3, 60, 100)])
def test_ranges_neighbours_matter(H, k, lo, hi):
    """one sequence more at either end of a range, an unused one or one of the enclosing range, changes the oracle's bits"""
    case = G.reference(H, "ranges")
    assert not G.same_bits(case["want"][k], G.oracle_train(H, case, k, seqs=case["seqs"][lo:hi]))


def test_ranges_poison(H):
    """The poison sequence in a model's range.  The oracle skips a sequence with a symbol >= M whole, so on its own the
    poison cannot change the oracle's bits (shown first); what a range that reaches it changes is that the entry point
    refuses the call, and that the sequences between change the training."""
    case = G.reference(H, "ranges")
    alone = case["seqs"][30:31] + [case["seqs"][G.POISON]]
    assert G.same_bits(case["want"][2], G.oracle_train(H, case, 2, seqs=alone))
    assert not G.same_bits(case["want"][2], G.oracle_train(H, case, 2, seqs=case["seqs"][30:G.POISON + 1]))
    reach = list(case["ranges"])
    reach[2] = (30, G.POISON + 1)
    with pytest.raises(e._lib.Ecoz2Error, match="model 2: symbol 60000 outside the codebook size 9"):
        e.hmm.train_grid(case["models"], case["seqs"], reach, case["eps"], case["val_auto"], case["maxit"])


def test_big_n_scratch_reaches_its_shape(H):
    case = G.reference(H, "big_n_scratch")
    assert [len(m[0]) for m in case["models"]] == [65, 141, 142, 200] and all(m[2].shape[1] == 8 for m in case["models"])
    assert all(hi - lo == 70 for lo, hi in case["ranges"]) and min(lo for lo, _hi in case["ranges"]) > 0
    assert G.merged_runs(case["ranges"])[0] == [(3, 283)]
    second = [i for i in range(70) if G.wg_slot(i, 70)[1] == 1]
    assert second == list(range(64, 70)) and [G.wg_slot(i, 70)[0] for i in second] == [0, 1, 2, 3, 4, 5]
    assert max(len(s) for s in case["seqs"]) <= 10
    for k in range(4):
        assert _check_bad(H, case, k, G.wg_slot) == {1: {"empty", "range", "emit"}}
        assert len(case["want"][k][3]) == 2
        first = G.slice_of(case, k, "grid_seqs")[:64]  # (a workgroup that stopped after its first sequence)
        assert not G.same_bits(case["want"][k], G.oracle_train(H, case, k, seqs=first))


def test_many_models_reaches_its_shape(H):
    case = G.many_reference(H)
    assert G.MANY_K == 65535 + 3 and G.grid_y_launches(G.MANY_K) == [65535, 3]
    # every model goes on to the M-step of iteration 0 (nothing stops before its second E-step), so the second launch
    # of the grid's M-step holds the last three
    assert all(len(w[3]) == 2 for w in case["want"])
    pairs = {G.many_pair_of(k) for k in range(G.MANY_K)}
    assert pairs == set(range(20)) and {G.many_pair_of(k) for k in range(65535, G.MANY_K)} <= pairs
    assert all(len(m[0]) == 1 and m[2].shape == (1, 4) for m, _r in case["pairs"])
    assert all(2 <= hi - lo <= 3 for _m, (lo, hi) in case["pairs"])
    # a model given its neighbour's class, or its neighbour's initial model, gets other bits: the 20 results are distinct,
    # and each differs from its initial model (an M-step ran)
    for i in range(20):
        assert not np.array_equal(G.bits(case["want"][i][2]), G.bits(case["pairs"][i][0][2]))
        for j in range(i):
            assert not G.same_bits(case["want"][i], case["want"][j]), (i, j)
