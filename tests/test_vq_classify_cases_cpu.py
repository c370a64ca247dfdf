"""The inputs of test_gpu_vq_classify.py held against the oracle alone (no device): the restated unit plan and report
against hand-written expectations, which edges of ecoz2_vq_classify's plan the file lengths reach, and that the planted
frames make a lost, doubled or misplaced frame show in the six digits of '%g' for every (file, codebook) pair."""
import os
import re

import numpy as np
import pytest

from tests import vq_classify_cases as vc


# ---- units() -------------------------------------------------------------------------------------------------------------
def test_units_at_1024():
    assert vc.units(vc.LENGTHS_36, 1024) == [
        # an exact fit: 493 + 531 == chunk, no flush in front of the 531-frame file (the leading empty file is a segment too)
        [(0, 0, 0, 0), (1, 0, 1, 0), (2, 0, 63, 1), (3, 0, 64, 64), (4, 0, 65, 128), (5, 0, 300, 193), (6, 0, 531, 493)],
        [(7, 0, 1, 0), (8, 0, 1023, 1)],    # 1024 + 1 > chunk: flushed; then 1 + 1023 == chunk, at an odd offset
        [(9, 0, 1024, 0)],                  # T == chunk is batched (whole), not cut
        [(10, 0, 1024, 0)], [(10, 1024, 1, 0)],
        [(11, 0, 1024, 0)], [(11, 1024, 1024, 0)], [(11, 2048, 452, 0)],
        [(12, 0, 0, 0)],                    # the empty file behind a cut one: a unit of no frames
    ]
    # values below the floor of 1024 frames plan alike
    assert vc.units(vc.LENGTHS_36, 1) == vc.units(vc.LENGTHS_36, 1024)


def test_units_at_1500():
    got = vc.units(vc.LENGTHS_36, 1500)
    assert got == [
        [(0, 0, 0, 0), (1, 0, 1, 0), (2, 0, 63, 1), (3, 0, 64, 64), (4, 0, 65, 128), (5, 0, 300, 193), (6, 0, 531, 493),
         (7, 0, 1, 1024)],                  # 1025 frames: the unit ends off a 64-frame block
        [(8, 0, 1023, 0)],                  # 1025 + 1023 > 1500
        [(9, 0, 1024, 0)],
        [(10, 0, 1025, 0)],                 # not cut any more; 1025 + 2500 > 1500
        [(11, 0, 1500, 0)], [(11, 1500, 1000, 0)],
        [(12, 0, 0, 0)],
    ]
    sizes = [sum(g[2] for g in un) for un in got]
    assert [n % 64 for n in sizes] == [1, 63, 0, 1, 28, 40, 0]


def test_units_unset_chunk_batches_everything():
    assert vc.chunk_frames(None) == 1 << 17
    (un,) = vc.units(vc.LENGTHS_36, None)
    assert [g[0] for g in un] == list(range(13)) and [g[2] for g in un] == list(vc.LENGTHS_36)
    assert [g[3] for g in un] == np.concatenate([[0], np.cumsum(vc.LENGTHS_36)[:-1]]).tolist()
    assert all(g[1] == 0 for g in un)


@pytest.mark.parametrize("chunk", [1024, 1500, None])
@pytest.mark.parametrize("Ts", [vc.LENGTHS_36, vc.LENGTHS_OTHER, vc.LENGTHS_TABLE])
def test_units_cover_every_frame_once(Ts, chunk):
    seen = [[] for _ in Ts]
    for un in vc.units(Ts, chunk):
        off = 0
        assert sum(g[2] for g in un) <= vc.chunk_frames(chunk)
        for k, t0, n, o in un:
            assert o == off
            off += n
            seen[k] += list(range(t0, t0 + n))
    assert [s == list(range(T)) for s, T in zip(seen, Ts)] == [True] * len(Ts)


def test_planted_places():
    assert vc.planted_places(0) == [] and vc.planted_places(1) == []
    assert vc.planted_places(63) == [0, 62] and vc.planted_places(1024) == [0, 1023]
    assert vc.planted_places(1025) == [0, 1023, 1024]
    assert vc.planted_places(2500) == [0, 1023, 1024, 1499, 1500, 2047, 2048, 2499]
    # every segment end of every plan of every case is a planted frame
    for name in vc.case_names():
        c = vc.case(name)
        for chunk in vc.CHUNKS:
            for un in vc.units(c.Ts, chunk):
                for k, t0, n, _o in un:
                    if c.Ts[k] >= 2:
                        assert t0 in c.planted[k] and t0 + n - 1 in c.planted[k], (name, chunk, k, t0, n)


# ---- report() ------------------------------------------------------------------------------------------------------------
def test_report_by_hand():
    """three codebooks (two of one class name apart: X, Y, X2), five files: a tie between codebooks 0 and 2 (the lower
    index wins, the ranking keeps them in index order), an empty file, classes in order of first appearance"""
    cbs = ["X", "Y", "X2"]
    paths = ["d/a.prd", "d/b.prd", "d/c.prd", "d/e.prd", "d/f.prd"]
    labels = ["Y", "X", "Y", "X2", "Y"]
    Ts = [3, 5, 0, 2, 1]
    scores = [[0.5, 0.25, 0.5], [1e-5, 123456789.0, 1e-5], [0.0, 0.0, 0.0], [2.0, 3.0, 2.0], [0.1, 1.0 / 3.0, 100.0]]
    want_table = ("\n"
                  "class                       tests  correct  percent\n"
                  "Y                               2        1   50.00%\n"
                  "X                               1        1  100.00%\n"
                  "X2                              1        0    0.00%\n"
                  "TOTAL                           4        2   50.00%\n")
    assert vc.report(cbs, paths, labels, Ts, scores, False) == want_table
    assert vc.report(cbs, paths, labels, Ts, scores, True) == (
        "d/e.prd: 'X2' classified as 'X'; ranked: X(2) X2(2) Y(3)\n"
        "d/f.prd: 'Y' classified as 'X'; ranked: X(0.1) Y(0.333333) X2(100)\n" + want_table)
    # '%g' beyond the fixed notation, and a list without a single frame
    assert vc.report(["X", "Y"], ["p"], ["Z"], [4], [[1e-5, 123456789.0]], True).startswith(
        "p: 'Z' classified as 'X'; ranked: X(1e-05) Y(1.23457e+08)\n")
    assert vc.report(["X"], ["p"], ["X"], [0], [[0.0]], True) == (
        "\nclass                       tests  correct  percent\nTOTAL                           0        0    0.00%\n")


def test_score_is_the_sum_in_frame_order():
    d = np.array([1.0 + 2.0 ** -30, 1e16, 1.0 + 2.0 ** -30, -1e16 + 2.0])
    assert vc.score(d) == (((2.0 ** -30 + (1e16 - 1.0)) + 2.0 ** -30) + (-1e16 + 2.0 - 1.0)) / 4
    assert vc.score(np.zeros(0)) == 0.0


# ---- the cases -----------------------------------------------------------------------------------------------------------
def test_routes_of_the_sizes():
    # prefiltered() against the sources: the prefilter's orders, the floor of quantize, the limits of prefilter_supports
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ecoz2rs_amd", "csrc")
    ncs = re.search(r"#define E2VQ_PRE_NC_LIST\(X\)((?: X\(\d+\))+)", open(os.path.join(csrc, "vq_device.h")).read()).group(1)
    orders = [int(n) - 1 for n in re.findall(r"\d+", ncs)]
    assert "int pre_min_M_quant = 256;" in open(os.path.join(csrc, "vq_session.h")).read()
    assert "return pre_has_nc(NC) && M >= 64 && M % 32 == 0 && M <= 8192;" in open(os.path.join(csrc, "vq_pre_images.hip")).read()
    assert [P for P in range(1, 201) if vc.prefiltered(P, 256)] == orders and 36 in orders and 40 in orders
    assert {int(n.rstrip("b")) for n in vc.M_ORDER_36} == set(vc.ROUTES_36)
    for M, route in vc.ROUTES_36.items():
        assert vc.prefiltered(36, M) == (route == "prefiltered"), M
    Ms = [int(n.rstrip("b")) for n in vc.M_ORDER_36]
    assert Ms != sorted(Ms)
    # two codebooks of one size side by side, with other contents
    c = vc.sizes_case(36)
    i = vc.M_ORDER_36.index("256")
    assert vc.M_ORDER_36[i + 1] == "256b" and c.cbs[i][1].shape == c.cbs[i + 1][1].shape
    assert not np.array_equal(c.cbs[i][1], c.cbs[i + 1][1])
    # plain <-> prefiltered both ways, a regrowth of the image buffer (above 2048) and a return below it, the capacity of the
    # codebook buffers grown by a larger M behind a smaller one
    pre = [vc.prefiltered(36, M) for M in Ms]
    assert (True, False) in zip(pre, pre[1:]) and (False, True) in zip(pre, pre[1:])
    assert Ms[0] == 2048 and Ms[-1] == 8192 and max(Ms[:Ms.index(4096)]) > 4096
    for P in vc.OTHER_ORDERS:
        assert [vc.prefiltered(P, int(n)) for n in vc.M_ORDER_OTHER] == [P in (20, 40), False, False]
    for seq in (vc.SWITCH_36, vc.SWITCH_48):
        assert seq[1:4] == ("256", "256b", "256") and seq[0] == "8" and seq[-1] == "256"
    assert vc.SWITCH_36[4:] == ("4096", "300", "2048", "8192", "8224", "64", "256")
    assert max(int(n.rstrip("b")) for n in vc.SWITCH_48) == 2048


@pytest.mark.parametrize("name", vc.case_names())
def test_planted_frames_show_in_six_digits(name):
    """for every (file, codebook) pair: a planted frame is at least 100 medians; dropped, counted twice or given to the
    neighbouring file it changes the '%g' text of the pair (and of the neighbour's pair); no two codebooks print alike"""
    c = vc.case(name)
    g = lambda x: "%g" % x
    nonempty = [k for k, T in enumerate(c.Ts) if T > 0]
    assert any(len(at) > 2 for at in c.planted) and any(T == 1 for T in c.Ts)
    for k in nonempty:
        T = c.Ts[k]
        texts = [g(s) for s in c.scores[k]]
        for i, t in enumerate(texts):
            same = [j for j, u in enumerate(texts) if u == t and j != i]
            assert same == ([j for j in c.tie if j != i] if i in c.tie else []), (name, k, i, texts)
        for i, d in enumerate(c.dmin[k]):
            x = (d - 1.0).tolist()
            if c.planted[k]:
                assert min(x[t] for t in c.planted[k]) >= 100.0 * float(np.median(d - 1.0)), (name, k, i)
            for t in c.planted[k]:
                dropped = sum_in_order(x[:t] + x[t + 1:]) / T
                twice = sum_in_order(x[:t + 1] + x[t:]) / T
                assert g(dropped) != texts[i] and g(twice) != texts[i], (name, k, i, t)
                # given away: the first half of a file's planted frames to the file in front, the others to the one behind
                pos = nonempty.index(k)
                q = pos - 1 if t < T / 2 else pos + 1
                if 0 <= q < len(nonempty):
                    n = nonempty[q]
                    xn = (c.dmin[n][i] - 1.0).tolist()
                    got = sum_in_order(xn + [x[t]] if q < pos else [x[t]] + xn) / c.Ts[n]
                    assert g(got) != g(c.scores[n][i]), (name, k, i, t, n)


def sum_in_order(xs):
    acc = 0.0
    for v in xs:
        acc += v
    return acc


def test_the_table_case_by_hand():
    c = vc.table_case()
    assert [cls for cls, _r in c.cbs] == ["C", "Bdup", "B", "A"] and c.tie == (1, 2)
    assert np.array_equal(c.cbs[1][1], c.cbs[2][1])
    assert c.Ts == list(vc.LENGTHS_TABLE) == [300, 700, 0, 1025, 65, 0, 64, 1, 0, 1500]
    assert [f[2] for f in c.files] == ["C", "A", "A", "B", "Bdup", "E", "A", "C", "E", "B"]
    paths = ["f%d" % k for k in range(len(c.files))]
    for k, row in enumerate(c.scores):
        assert row[1] == row[2]
    best = [min(range(4), key=lambda i: row[i]) if T else None for row, T in zip(c.scores, c.Ts)]  # (first minimum)
    #        C  A  -     B  Bdup -     A(of C) C(of A) -  B
    assert best == [0, 3, None, 1, 1, None, 0, 3, None, 1]
    table = ("\n"
             "class                       tests  correct  percent\n"
             "C                               2        1   50.00%\n"
             "A                               2        1   50.00%\n"
             "B                               2        0    0.00%\n"
             "Bdup                            1        1  100.00%\n"
             "TOTAL                           7        3   42.86%\n")
    assert c.report(paths, False) == table
    ranked = c.report(paths, True)
    assert ranked.endswith(table)
    lines = ranked[:-len(table)].splitlines()
    assert [l.split(";")[0] for l in lines] == ["f3: 'B' classified as 'Bdup'", "f6: 'A' classified as 'C'",
                                                "f7: 'C' classified as 'A'", "f9: 'B' classified as 'Bdup'"]
    assert [[w.split("(")[0] for w in l.split("ranked: ")[1].split()] for l in lines] == [
        ["Bdup", "B", "A", "C"], ["C", "A", "Bdup", "B"], ["A", "C", "Bdup", "B"], ["Bdup", "B", "A", "C"]]
    # in the CLI's order (paths sorted: A, B, Bdup, C) B takes the tie
    cli = c.report(paths, True, cb_order=[3, 2, 1, 0])
    assert "f4: 'Bdup' classified as 'B'; ranked: B(" in cli and "'B' classified" not in cli
    assert "B                               2        2  100.00%\n" in cli and "TOTAL                           7        4   57.14%\n" in cli


def test_the_switching_steps():
    for P in (36, 40, 48):
        steps = vc.switch_steps(P)
        seq = vc.SWITCH_48 if P == 48 else vc.SWITCH_36
        assert [s[0] for s in steps] == list(seq)
        assert [len(s[2]) for s in steps] == [vc.SWITCH_T[q % 4] for q in range(len(seq))]
        assert all(s[1].shape == (int(s[0].rstrip("b")), P + 1) and len(s[3]) == len(s[4]) == len(s[2]) for s in steps)
        # a stale codebook would be seen: the same frames fall into other cells and other distortions under 256 and 256b
        a, b = steps[1], steps[2]
        sym_b_on_a_frames = vc.oracle().quantize(vc.oracle().reflections_to_cq(b[1]), a[2])
        assert not np.array_equal(sym_b_on_a_frames[1], a[4])


def test_refusals_before_the_device(tmp_path, capfd):
    """what ecoz2_vq_classify refuses before it opens a device: no codebook, a codebook of another order, a predictor
    file of another order (behind a long one) -- the library's message, and nothing on stdout"""
    import ecoz2rs_amd as e

    c, other = vc.table_case(), vc.sizes_case(20)
    cbs, prds = c.write(tmp_path)
    cb20, prd20 = str(tmp_path / "p20.cbook"), str(tmp_path / "p20.prd")
    e.formats.write_cbook(cb20, "B", other.cbs[1][1])
    e.formats.write_prd(prd20, "B", other.files[1][3])
    capfd.readouterr()
    for cb_list, prd_list, message in (
            ([], prds, "ecoz2_vq_classify: bad arguments"),
            (cbs + [cb20], prds, cb20 + ": prediction order differs from the first codebook"),
            (cbs, prds + [prd20], prd20 + ": prediction order 20 differs from the codebooks' 36")):
        with pytest.raises(e.Ecoz2Error) as err:
            e.vq_classify(cb_list, prd_list, show_ranked=True)
        assert str(err.value) == message
    assert capfd.readouterr().out == ""
