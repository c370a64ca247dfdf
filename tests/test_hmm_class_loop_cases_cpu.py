"""the shared inputs of test_gpu_hmm_class_loop_shapes.py and test_gpu_hmm_trans_posteriors_shapes.py
(tests/hmm_class_loop_cases.py), CPU side: the restated constants and the LDS sums of the five launchers against hmm_device.h
and the .hip sources; the body and the placement of lA (and lt) that every row of SHAPES reaches in each decoder; the
instantiation and the bytes of dynamic LDS that every row, event set and random set of --grammar-posteriors (4.8.13) reaches
(the restatement at those rows is held against extended precision in test_hmm_trans_posteriors_cpu.py); on the restatements alone, what makes a row worth running -- its path visits many classes in many slots, the
last one among them, and a session over it decides frames after every block --; the vectorised restatements against their
literal forms on the event streams, and the status of each; the seeded random sets.  For test_gpu_hmm_grammar_shapes.py: the LDS
sums and decision orders of the two grammar trainers (4.8.14, 4.8.16) and of the grammar session (4.8.15) against their
launchers, the layout and bytes of every row of GRAMMAR_SHAPES in each of the three kernels, every instantiation and count-table
route reached (above 64 KB where one can be), the status of the event streams under the trainers' restatements, and that the
session's restatement delivers frames before close at every row."""
import os
import re

import numpy as np
import pytest

from . import hmm_class_loop_cases as cases
from . import hmm_loop_em_restatement as RLE
from . import hmm_posterior_restatement as RP
from . import hmm_segment_restatement as R
from . import hmm_segment_trans_restatement as RT
from . import hmm_transitions_em_restatement as RTE
from . import hmm_viterbi_restatement as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
NINF = float("-inf")


def _source(name):
    return open(os.path.join(CSRC, name)).read()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- the restated constants and sums ---------------------------------------------------------------------------------------------
def test_the_restated_constants_are_the_sources():
    dev = _source("hmm_device.h")
    lds = re.search(r"constexpr\s+size_t\s+SEG_LDS_BYTES\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", dev)
    assert cases.SEG_LDS_BYTES == int(lds.group(1)) * int(lds.group(2))
    for name in ("SEG_MAX_WAVES", "SEG_MAX_SUM_N"):
        assert getattr(cases, name) == int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, dev).group(1)), name
    stream = _source("hmm_segment_stream.hip")
    assert cases.COALESCE_THREADS == int(re.search(r"constexpr\s+int\s+COALESCE_THREADS\s*=\s*(\d+)\s*;", stream).group(1))
    assert "constexpr int COALESCE_PER_THREAD = SEG_MAX_SUM_N / COALESCE_THREADS;" in stream
    assert cases.COALESCE_PER_THREAD == 4
    # the one Pair struct (hmm_segment_trans.hip takes it from the header too): a double and two ints, no padding between or behind them
    for name in ("hmm_segment_common.h",):
        pair = re.search(r"struct\s+Pair\s*\{[^\n]*\n(.*?)\};", _source(name), re.S)
        size = sum({"double": 8, "int": 4}[typ] * len(names.split(",")) for typ, names in re.findall(r"\b(double|int)\s+([^;]+);", pair.group(1)))
        assert cases.PAIR_BYTES == size == 16, name
    assert '#include "hmm_segment_common.h"' in _source("hmm_segment_trans.hip")


def test_no_hmm_unit_defines_the_shared_lane_helpers_again():
    # hmm_lane.h holds them once (the chains are the bit-exactness contract); a new unit includes the header
    shared = ("bcast", "lane_read", "scale_step", "block_sum", "slot_sum", "slots_sum", "chain_sum", "unit_sum", "chain_col",
              "chain_row", "chain_col_mass", "chain_row_pi")
    define = re.compile(r"__device__[^;{}()]*?\b(?:double|void|ChainPair)\s+(%s)\s*\(" % "|".join(shared))
    assert sorted(set(define.findall(_source("hmm_lane.h")))) == sorted(set(shared) - {"unit_sum"})
    units = sorted(n for n in os.listdir(CSRC) if re.fullmatch(r"hmm_\w+\.hip", n))
    assert len(units) >= 13
    for name in units:
        src = _source(name)
        assert not define.findall(src), (name, define.findall(src))
        assert not re.search(r"\bstruct\s+Pair\b", src), name
    assert len(re.findall(r"\bstruct\s+Pair\s*\{", _source("hmm_segment_common.h"))) == 1


def test_the_restated_lds_sums_are_the_launchers():
    body = lambda name, fn: re.search(r"size_t %s\([^)]*\)\s*\{(.*?)\n\s*\}" % fn, _source(name), re.S).group(1)
    seg = "(size_t)2 * SEG_MAX_WAVES * sizeof(Pair) + (a_lds ? (size_t)pl.a_words * 8 : 0) + (looped ? (size_t)2 * pl.sumN * 8 : 0)"
    assert seg in body("hmm_segment.hip", "segment_lds_bytes") and seg in body("hmm_segment_stream.hip", "stream_lds_bytes")
    assert "(size_t)2 * SEG_MAX_WAVES * sizeof(double) + (a_lds ? (size_t)pl.a_words * 8 : 0)" in body("hmm_posterior.hip", "posteriors_lds_bytes")
    trans = body("hmm_segment_trans.hip", "trans_lds_bytes")
    assert "(size_t)SEG_MAX_WAVES * sizeof(Pair) + (size_t)2 * pl.K * 8 + (a_lds ? (size_t)pl.a_words * 8 : 0) +" in trans
    assert "(lt_lds ? (size_t)pl.K * pl.K * 8 : 0)" in trans
    # lA is placed first and lt takes what is left; the posteriors' A has an odd leading dimension
    layout = _source("hmm_segment_trans.hip")
    assert "*a_lds = trans_lds_bytes(pl, true, false) <= SEG_LDS_BYTES;" in layout
    assert "*lt_lds = trans_lds_bytes(pl, *a_lds, true) <= SEG_LDS_BYTES;" in layout
    assert "int posteriors_a_ld(int N) { return N | 1; }" in _source("hmm_class_loop.cpp")
    # every launcher raises the limit of dynamic LDS above 64 KB, and the first three choose lA by the same comparison
    for name in ("hmm_segment.hip", "hmm_segment_stream.hip", "hmm_posterior.hip", "hmm_segment_trans.hip"):
        src = _source(name)
        assert "if (lds > 64 * 1024 &&" in src and "hipFuncAttributeMaxDynamicSharedMemorySize" in src, name
    assert cases.LDS_OPT_IN == 64 * 1024
    assert "const bool a_lds = segment_lds_bytes(pl, looped, true) <= SEG_LDS_BYTES;" in _source("hmm_segment.hip")
    assert "const bool a_lds = stream_lds_bytes(pl, looped, true) <= SEG_LDS_BYTES;" in _source("hmm_segment_stream.hip")
    assert "return posteriors_lds_bytes(pl, true) <= SEG_LDS_BYTES;" in _source("hmm_posterior.hip")
    assert "*looped = slots > e2hmm::SEG_MAX_WAVES || (body && strcmp(body, \"looped\") == 0);" in _source("hmm_class_loop.cpp")
    # the fifth: --grammar-posteriors counts doubles (partials of two parities, S / R of two steps, pi, A, w and wT); A goes
    # in first, then both matrices; the packing is the posteriors' (odd leading dimension)
    src = _source("hmm_posterior_trans.hip")
    post_trans = body("hmm_posterior_trans.hip", "post_trans_lds_bytes")
    assert "return ((size_t)2 * SEG_MAX_WAVES + (size_t)2 * pl.K + (size_t)pl.sumN + (a_lds ? (size_t)pl.a_words : 0) +" in post_trans
    assert "(w_lds ? (size_t)2 * pl.K * pl.K : 0)) * sizeof(double);" in post_trans
    assert "*a_lds = post_trans_lds_bytes(pl, true, false) <= SEG_LDS_BYTES;" in src
    assert "*w_lds = post_trans_lds_bytes(pl, *a_lds, true) <= SEG_LDS_BYTES;" in src
    assert "if (lds > 64 * 1024 &&" in src and "hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEG_LDS_BYTES) != hipSuccess)" in src
    assert "if (lds > SEG_LDS_BYTES) return 1;" in src
    device = _source("hmm_class_loop.cpp")
    at = device.index("int trans_posteriors_device(")
    assert "const SegPacking pk = pack_slots(lm.Ns, posteriors_a_ld);" in device[at:at + 600]
    assert cases.trans_posteriors_lds_bytes(3, 12, 68, True, True) == (32 + 6 + 12 + 68 + 18) * 8


# ---- where every row goes --------------------------------------------------------------------------------------------------------
# name: decoder: (body, lA in LDS, lt in LDS or None, more than 64 KB of dynamic LDS); only the decoders the GPU file runs the row through
ROUTES = {
    "64x64": {"segment": ("looped", False, None, True), "stream": ("looped", False, None, True)},
    "1x4096": {"segment": ("looped", True, None, True)},
    "1x1024": {"segment": ("resident", True, None, False), "posteriors": ("resident", True, None, False),
               "trans": ("resident", True, False, False)},
    "33x20": {"segment": ("looped", False, None, False), "stream": ("looped", False, None, False)},
    "40_1x24_x14": {"segment": ("resident", False, None, False), "posteriors": ("resident", False, None, False)},
}


@pytest.mark.parametrize("name", list(cases.SHAPES))
def test_every_row_reaches_the_body_and_the_placement_its_comment_names(name):
    Ns = cases.SHAPES[name][0]
    assert sum(Ns) <= cases.SEG_MAX_SUM_N
    for decoder, (body, a_lds, lt_lds, big) in ROUTES[name].items():
        r = cases.route(decoder, Ns)
        assert (r["body"], r["a_lds"], r["lt_lds"], r["lds"] > cases.LDS_OPT_IN) == (body, a_lds, lt_lds, big), (decoder, r)
        assert r["lds"] <= cases.SEG_LDS_BYTES
    slots = cases.slots_of(Ns)
    assert slots == {"64x64": 64, "1x4096": 64, "1x1024": 16, "33x20": 20, "40_1x24_x14": 14}[name]
    if name in ("64x64", "1x4096"):  # the documented maximum: four turns to each of a looped workgroup's 16 waves
        assert sum(Ns) == cases.SEG_MAX_SUM_N and slots == 4 * cases.SEG_MAX_WAVES
        assert 2 * sum(Ns) * 8 == cases.LDS_OPT_IN  # (d of two steps alone is 64 KB: the pairs put the sum above it)
    if name == "40_1x24_x14":  # (the row of test_gpu_hmm_segment_trans.py, where both lA and lt are read from global memory)
        assert cases.route("trans", Ns)["a_lds"] is False and cases.route("trans", Ns)["lt_lds"] is False


def test_the_event_models_reach_both_bodies_and_lA_in_both_places():
    small, mid, wide = ([len(m[0]) for m in cases.event_models(name)] for name in ("5_3_4", "64x6", "64x17"))
    assert small == [5, 3, 4] and mid == [64] * 6 and wide == [64] * 17
    for decoder in ("segment", "stream"):  # k_hmm_segment<LOOPED, A_LDS> and k_hmm_segment_stream<LOOPED, A_LDS>
        assert cases.route(decoder, small)["body"] == "resident" and cases.route(decoder, small)["a_lds"]      # <false, true>
        assert cases.route(decoder, small, looped=True) == dict(body="looped", a_lds=True, lt_lds=None,
                                                               lds=512 + 50 * 8 + 2 * 12 * 8)                  # <true, true>
        assert cases.route(decoder, mid)["body"] == "resident" and not cases.route(decoder, mid)["a_lds"]      # <false, false>
        assert cases.route(decoder, wide)["body"] == "looped" and not cases.route(decoder, wide)["a_lds"]      # <true, false>
    for models in (cases.event_models(name) for name in cases.EVENT_NS):
        assert all(not B[:, cases.DEAD].any() and (np.delete(B, cases.DEAD, axis=1) > 0).all() and (A > 0).all() and (pi > 0).all()
                   for pi, A, B in models)
    # the posteriors' zero fill of a failed stream, x = threadIdx.x; x < T * K; x += blockDim.x, takes 7 turns there
    assert cases.EVENT_T * len(small) > 6 * 64 * cases.slots_of(small)


# ---- --grammar-posteriors: the instantiation and the dynamic LDS of every row --------------------------------------------------
# name: (K, slots, A in LDS, w and wT in LDS, bytes of dynamic LDS) -- k_hmm_loop_posteriors_trans<A_LDS, W_LDS>
TRANS_POSTERIORS_ROUTES = {
    "64x3": (3, 3, True, True, 101824),
    "64x6_1x84": (90, 8, False, True, 135040),
    "40_1x24_x6": (150, 6, True, False, 85600),
    "64x4_1x768": (772, 16, True, False, 160064),
    "1x1024": (1024, 16, True, False, 33024),
    "40_1x24_x14": (350, 14, False, False, 13024),
    "64x8_1x512": (520, 16, False, False, 16768),
}


def test_the_rows_of_the_grammar_posteriors_reach_every_instantiation_and_the_opt_in_of_three():
    assert list(cases.TRANS_POSTERIORS_SHAPES) == list(TRANS_POSTERIORS_ROUTES) and cases.TRANS_POSTERIORS_T == 130
    seen, opted = set(), set()
    for name, (K, slots, a_lds, w_lds, lds) in TRANS_POSTERIORS_ROUTES.items():
        Ns = cases.TRANS_POSTERIORS_SHAPES[name][0]
        r = cases.route("trans_posteriors", Ns)
        assert (len(Ns), cases.slots_of(Ns), r["a_lds"], r["w_lds"], r["lds"]) == (K, slots, a_lds, w_lds, lds), (name, r)
        assert r["body"] == "resident" and lds <= cases.SEG_LDS_BYTES and sum(Ns) <= cases.SEG_MAX_SUM_N
        seen.add((a_lds, w_lds))
        if lds > cases.LDS_OPT_IN:
            opted.add((a_lds, w_lds))
    assert seen == {(True, True), (False, True), (True, False), (False, False)}
    # <false, false> holds the partials, S / R and pi alone: at most (32 + 2 * 1024 + 4096) * 8 bytes, below the opt-in
    assert opted == {(True, True), (False, True), (True, False)}
    assert cases.trans_posteriors_lds_bytes(1024, cases.SEG_MAX_SUM_N, 0, False, False) < cases.LDS_OPT_IN
    assert cases.SEG_LDS_BYTES - TRANS_POSTERIORS_ROUTES["64x4_1x768"][4] == 3776
    # the one-class slots of "64x8_1x512" read their chains by readlane, next to eight packed slots of 64 classes each
    assert cases.one_class_slot_next_to_packed(cases.TRANS_POSTERIORS_SHAPES["64x8_1x512"][0])
    # (the largest launch of the kernel's own GPU file, "21_22_64", stays below the opt-in)
    assert cases.route("trans_posteriors", [21, 22, 64])["lds"] == 42160


def test_the_event_sets_of_the_grammar_posteriors_reach_every_instantiation():
    want = {"5_3_4": (True, True, False), "64x6": (False, True, False), "64x3": (True, True, True),
            "40_1x24_x14": (False, False, False)}
    assert cases.TRANS_POSTERIORS_EVENT_SETS == tuple(want)
    for name, (a_lds, w_lds, big) in want.items():
        Ns = [len(m[0]) for m in cases.event_models(name)]
        assert Ns == list(cases.EVENT_NS[name])
        r = cases.route("trans_posteriors", Ns)
        assert (r["a_lds"], r["w_lds"], r["lds"] > cases.LDS_OPT_IN) == (a_lds, w_lds, big), (name, r)
    assert cases.route("trans_posteriors", cases.EVENT_NS["64x6"])["lds"] == 4000
    # the zero fill of a failed stream, x = threadIdx.x; x < T * K; x += blockDim.x: 130 x 350 entries by 896 threads
    Ns = cases.EVENT_NS["40_1x24_x14"]
    assert (cases.EVENT_T * len(Ns), 64 * cases.slots_of(Ns)) == (45500, 896)
    assert [cases.event_status(k, "trans_posteriors") for k in cases.EVENT_KINDS] == [0, 2, 1, 1, 2]


def test_the_random_sets_take_the_grammar_posteriors_above_64_kb_in_two_instantiations():
    routes = [cases.route("trans_posteriors", row["Ns"]) for row in cases.random_shapes(cases.RANDOM_SEED, resident_only=True)]
    assert len(routes) == 12
    for i in (1, 8, 11):
        assert routes[i]["a_lds"] and routes[i]["w_lds"] and routes[i]["lds"] > cases.LDS_OPT_IN, (i, routes[i])
    assert (routes[0]["a_lds"], routes[0]["w_lds"], routes[0]["lds"]) == (True, False, 161120)
    print([(r["a_lds"], r["w_lds"], r["lds"]) for r in routes])


def test_the_neighbour_row_takes_segment_trans_above_64_kb_with_lA_global():
    r = cases.route("trans", cases.TRANS_POSTERIORS_SHAPES["64x6_1x84"][0])
    assert (r["a_lds"], r["lt_lds"], r["lds"]) == (False, True, 66496) and r["lds"] > cases.LDS_OPT_IN
    models, stream, lt = cases.trans_posteriors_shape("64x6_1x84")
    want = RT.segment_trans(models, stream, [0, len(stream)], lt)
    assert want["status"].tolist() == [0] and want["entered"].sum() >= 10  # (a path of one segment would read little of lt)


# ---- the grammar trainers and the grammar session: the sums, and the layout and bytes of every row ----------------------------
def test_the_restated_lds_sums_of_the_grammar_kernels_are_the_launchers():
    body = lambda name, fn: re.search(r"size_t %s\([^)]*\)\s*\{(.*?)\n\s*\}" % fn, _source(name), re.S).group(1)
    # 4.8.14: doubles (partials of two parities, S / R of two steps, pi, the C table, A, w and wT); the order c, a, w
    src = _source("hmm_trans_estep.hip")
    te = body("hmm_trans_estep.hip", "trans_estep_lds_bytes")
    assert "return ((size_t)2 * SEG_MAX_WAVES + (size_t)2 * pl.K + (size_t)pl.sumN + (c_lds ? (size_t)2 * pl.K * pl.K : 0) +" in te
    assert "(a_lds ? (size_t)pl.a_words : 0) + (w_lds ? (size_t)2 * pl.K * pl.K : 0)) * sizeof(double);" in te
    assert "if (!c_forced) *c_lds = trans_estep_lds_bytes(pl, true, false, false) <= SEG_LDS_BYTES;" in src
    assert "*a_lds = trans_estep_lds_bytes(pl, *c_lds, true, false) <= SEG_LDS_BYTES;" in src
    assert "*w_lds = trans_estep_lds_bytes(pl, *c_lds, *a_lds, true) <= SEG_LDS_BYTES;" in src
    assert src.index("*c_lds = trans_estep_lds_bytes") < src.index("*a_lds = trans_estep_lds_bytes") < src.index("*w_lds = trans_estep_lds_bytes")
    # 4.8.16: the AN table (two words a cell of A) before the C table; the order an, c (with the grammar table alone), a, w
    loop = _source("hmm_loop_estep.hip")
    le = body("hmm_loop_estep.hip", "loop_estep_lds_bytes")
    assert "return ((size_t)2 * SEG_MAX_WAVES + (size_t)2 * pl.K + (size_t)pl.sumN + (an_lds ? (size_t)2 * pl.a_words : 0) +" in le
    assert "(c_lds ? (size_t)2 * pl.K * pl.K : 0) + (a_lds ? (size_t)pl.a_words : 0) + (w_lds ? (size_t)2 * pl.K * pl.K : 0)) *" in le
    assert "sizeof(double);" in le
    order = ["if (!an_forced) *an_lds = loop_estep_lds_bytes(pl, true, false, false, false) <= SEG_LDS_BYTES;",
             "if (!gram) *c_lds = false;",
             "else if (!c_forced) *c_lds = loop_estep_lds_bytes(pl, *an_lds, true, false, false) <= SEG_LDS_BYTES;",
             "*a_lds = loop_estep_lds_bytes(pl, *an_lds, *c_lds, true, false) <= SEG_LDS_BYTES;",
             "*w_lds = loop_estep_lds_bytes(pl, *an_lds, *c_lds, *a_lds, true) <= SEG_LDS_BYTES;"]
    at = [loop.index(line) for line in order]
    assert at == sorted(at)
    assert "if (!gram) c_lds = false;" in loop  # (the launcher's own: a call without the table has no C table in LDS)
    # 4.8.15: segment_trans_layout decides (its sum holds the pairs), the launch is without them
    stream = _source("hmm_segment_trans_stream.hip")
    assert "segment_trans_layout(pl, &a_lds, &lt_lds);" in stream
    assert ("const size_t lds = (size_t)2 * pl.K * 8 + (a_lds ? (size_t)pl.a_words * 8 : 0) + (lt_lds ? (size_t)pl.K * pl.K * 8 : 0);"
            in stream)
    for name, text in (("hmm_trans_estep.hip", src), ("hmm_loop_estep.hip", loop), ("hmm_segment_trans_stream.hip", stream)):
        assert "if (lds > 64 * 1024 &&" in text and "hipFuncAttributeMaxDynamicSharedMemorySize" in text, name
        assert "(int)SEG_LDS_BYTES) != hipSuccess)" in text and "if (lds > SEG_LDS_BYTES) return 1;" in text, name
    # both trainers pack with the posteriors' odd leading dimension, the session with the decoder's N x N
    assert "tp.pk = pack_slots(Ns, posteriors_a_ld);" in _source("hmm_trans_train.cpp")
    assert "lp.pk = pack_slots(Ns, posteriors_a_ld);" in _source("hmm_loop_train.cpp")
    assert cases.trans_estep_lds_bytes(3, 12, 68, True, True, True) == (32 + 6 + 12 + 18 + 68 + 18) * 8
    assert cases.loop_estep_lds_bytes(3, 12, 68, True, True, True, True) == (32 + 6 + 12 + 136 + 18 + 68 + 18) * 8
    assert cases.trans_stream_lds_bytes(3, 50, True, True) == (6 + 50 + 9) * 8


# name: k_hmm_trans_estep (c, a, w, bytes), k_hmm_loop_estep with the table (an, c, a, w, bytes) and without it (an, a, w,
# bytes), k_hmm_segment_trans_stream (a, lt, bytes)
T_, F_ = True, False
GRAMMAR_ROUTES = {
    "64x3": ((T_, T_, T_, 101968), (F_, T_, T_, T_, 101968), (F_, T_, T_, 101824), (T_, T_, 98424)),
    "64x6_1x84": ((T_, F_, F_, 135040), (F_, T_, F_, F_, 135040), (F_, F_, T_, 135040), (F_, T_, 66240)),
    "40_1x24_x6": ((F_, T_, F_, 85600), (F_, F_, T_, F_, 85600), (F_, T_, F_, 85600), (T_, F_, 80352)),
    "64x4_1x768": ((F_, T_, F_, 160064), (F_, F_, T_, F_, 160064), (F_, T_, F_, 160064), (T_, F_, 149568)),
    "1x1024": ((F_, T_, F_, 33024), (T_, F_, T_, F_, 49408), (T_, T_, F_, 49408), (T_, F_, 24576)),
    "40_1x24_x14": ((F_, F_, F_, 13024), (F_, F_, F_, F_, 13024), (F_, F_, F_, 13024), (F_, F_, 5600)),
    "64x8_1x512": ((F_, F_, F_, 16768), (F_, F_, F_, F_, 16768), (F_, F_, F_, 16768), (F_, F_, 8320)),
    "64x2": ((T_, T_, T_, 68000), (T_, T_, F_, T_, 134560), (T_, F_, T_, 134496), (T_, T_, 65600)),
    "1x71": ((T_, T_, T_, 163840), (T_, T_, T_, F_, 84320), (T_, T_, T_, 84320), (T_, T_, 42032)),
    "1x80": ((T_, T_, F_, 105216), (T_, T_, T_, F_, 106496), (T_, T_, T_, 106496), (T_, T_, 53120)),
    "64_1x64": ((T_, T_, F_, 103712), (T_, T_, F_, F_, 137504), (T_, T_, F_, 103696), (T_, T_, 68120)),
    "64x2_1x60": ((T_, T_, F_, 131296), (T_, F_, F_, F_, 136832), (T_, F_, F_, 136832), (T_, T_, 97760)),
    "64x3_1x64": ((T_, F_, T_, 147024), (F_, T_, F_, T_, 147024), (F_, T_, F_, 103728), (T_, T_, 135800)),
}


def _grammar_routes(name):
    Ns = cases.GRAMMAR_SHAPES[name][0]
    te, le, lp, ts = (cases.route("trans_estep", Ns), cases.route("loop_estep", Ns), cases.route("loop_estep", Ns, gram=False),
                      cases.route("trans_stream", Ns))
    return ((te["c_lds"], te["a_lds"], te["w_lds"], te["lds"]), (le["an_lds"], le["c_lds"], le["a_lds"], le["w_lds"], le["lds"]),
            (lp["an_lds"], lp["a_lds"], lp["w_lds"], lp["lds"]), (ts["a_lds"], ts["lt_lds"], ts["lds"]))


def test_every_row_of_the_grammar_shapes_reaches_the_layouts_and_bytes_its_comment_names():
    assert list(cases.GRAMMAR_SHAPES) == list(GRAMMAR_ROUTES)
    assert list(cases.GRAMMAR_SHAPES)[:7] == list(cases.TRANS_POSTERIORS_SHAPES)
    for name, (Ns, M, T) in cases.GRAMMAR_SHAPES.items():
        assert _grammar_routes(name) == GRAMMAR_ROUTES[name], (name, _grammar_routes(name))
        assert max(r[-1] for r in GRAMMAR_ROUTES[name]) <= cases.SEG_LDS_BYTES
        assert cases.slots_of(Ns) <= cases.SEG_MAX_WAVES and sum(Ns) <= cases.SEG_MAX_SUM_N and 66 <= T <= cases.TRANS_POSTERIORS_T
        if name in cases.TRANS_POSTERIORS_SHAPES:  # the same models, stream and prices as the posteriors' row
            assert (Ns, M) == cases.TRANS_POSTERIORS_SHAPES[name] and T == cases.TRANS_POSTERIORS_T
        else:
            assert M == 64
        assert cases.route("loop_estep", Ns, gram=False)["c_lds"] is None
    # the cap exactly: no launch of the project asks for more dynamic LDS than "1x71" in k_hmm_trans_estep<true, true>
    assert GRAMMAR_ROUTES["1x71"][0][3] == cases.SEG_LDS_BYTES == 160 * 1024
    assert cases.trans_estep_lds_bytes(72, 72, 72, True, True, True) > cases.SEG_LDS_BYTES  # (one class more and w leaves LDS)
    # (the largest launches of the kernels' own GPU files, at "21_22_64", stay below the opt-in)
    assert cases.route("trans_estep", [21, 22, 64])["lds"] == 42304 and cases.route("trans_stream", [21, 22, 64])["lds"] == 40288
    assert cases.route("loop_estep", [21, 22, 64])["lds"] > cases.LDS_OPT_IN and cases.route("loop_estep", [21, 22, 64])["a_lds"]


def test_the_grammar_shapes_reach_every_instantiation_route_and_the_opt_in_where_one_can_be():
    big = lambda lds: lds > cases.LDS_OPT_IN
    te = {(r[0][1], r[0][2], r[0][0], big(r[0][3])) for r in GRAMMAR_ROUTES.values()}  # (A_LDS, W_LDS, c_lds, above 64 KB)
    # k_hmm_trans_estep<A_LDS, W_LDS>: all four, each with the C table in LDS above 64 KB ...
    assert {(a, w, True, True) for a in (T_, F_) for w in (T_, F_)} <= te
    # ... and with the table in global memory: <true, false> above 64 KB, <false, false> below it (partials, S / R and pi
    # alone stay below the opt-in); W in LDS next to a global table the rule cannot produce (C goes in first and is as large)
    assert (T_, F_, F_, True) in te and (F_, F_, F_, False) in te and not any(w and not c for _a, w, c, _b in te)
    assert cases.trans_estep_lds_bytes(1024, cases.SEG_MAX_SUM_N, 0, False, False, False) < cases.LDS_OPT_IN
    # (the forced route the GPU file adds at "64x3" and "1x80": <true, true> with the table in global memory, at "1x80" w
    # takes the room the table leaves)
    for name, want in (("64x3", (F_, T_, T_, 101824)), ("1x80", (F_, T_, T_, 105216))):
        r = cases.route("trans_estep", cases.GRAMMAR_SHAPES[name][0], c=False)
        assert (r["c_lds"], r["a_lds"], r["w_lds"], r["lds"]) == want, (name, r)
    r = cases.route("trans_estep", cases.GRAMMAR_SHAPES["40_1x24_x6"][0], c=True)  # forced into LDS: refused by the host
    assert r["lds"] == 365728 > cases.SEG_LDS_BYTES
    # k_hmm_loop_estep<A_LDS, W_LDS, GRAM>: all eight, and every (an, c) the rule can produce, each above 64 KB but <f, f, *>
    # without a table in LDS
    le = {(r[1][2], r[1][3], True, big(r[1][4])) for r in GRAMMAR_ROUTES.values()}
    le |= {(r[2][1], r[2][2], False, big(r[2][3])) for r in GRAMMAR_ROUTES.values()}
    assert {(a, w, g, True) for a in (T_, F_) for w in (T_, F_) for g in (T_, F_)} <= le
    anc = {(r[1][0], r[1][1], big(r[1][4])) for r in GRAMMAR_ROUTES.values()}
    assert {(an, c, True) for an in (T_, F_) for c in (T_, F_)} <= anc
    assert GRAMMAR_ROUTES["64x2"][1][:4] == (T_, T_, F_, T_)  # the AN table in LDS (leading dimension N | 1) while A is global
    assert {(r[1][0], r[1][2]) for r in GRAMMAR_ROUTES.values()} == {(a, b) for a in (T_, F_) for b in (T_, F_)}
    # C in LDS with w global, and C global with w global, in both trainers
    assert any(r[0][0] and not r[0][2] for r in GRAMMAR_ROUTES.values()) and any(r[1][1] and not r[1][3] for r in GRAMMAR_ROUTES.values())
    # k_hmm_segment_trans_stream<A_LDS, LT_LDS>: all four, three of them above 64 KB (<false, false> holds E of two steps alone)
    ts = {(r[3][0], r[3][1], big(r[3][2])) for r in GRAMMAR_ROUTES.values()}
    assert {(T_, T_, True), (F_, T_, True), (T_, F_, True), (F_, F_, False)} <= ts
    assert cases.trans_stream_lds_bytes(4096, 0, False, False) == cases.LDS_OPT_IN  # (not above it)
    # the forced routes of the loop E-step at "64x2": each changes the layout
    Ns = cases.GRAMMAR_SHAPES["64x2"][0]
    free, an_g, c_g = cases.route("loop_estep", Ns), cases.route("loop_estep", Ns, an=False), cases.route("loop_estep", Ns, c=False)
    pick = lambda r: (r["an_lds"], r["c_lds"], r["a_lds"], r["w_lds"], r["lds"])
    assert pick(free) == (T_, T_, F_, T_, 134560) and pick(an_g) == (F_, T_, T_, T_, 68000) and pick(c_g) == (T_, F_, F_, T_, 134496)


def test_the_event_sets_of_the_grammar_trainers_and_the_status_of_every_event_stream():
    assert cases.GRAMMAR_EVENT_SETS == cases.TRANS_POSTERIORS_EVENT_SETS + ("64x2",)
    want = {"5_3_4": ((T_, T_, T_), (T_, T_, T_, T_)), "64x6": ((T_, F_, T_), (F_, T_, F_, T_)), "64x3": ((T_, T_, T_), (F_, T_, T_, T_)),
            "40_1x24_x14": ((F_, F_, F_), (F_, F_, F_, F_)), "64x2": ((T_, T_, T_), (T_, T_, F_, T_))}
    for name in cases.GRAMMAR_EVENT_SETS:
        Ns = [len(m[0]) for m in cases.event_models(name)]
        assert Ns == list(cases.EVENT_NS[name])
        te, le = cases.route("trans_estep", Ns), cases.route("loop_estep", Ns)
        assert ((te["c_lds"], te["a_lds"], te["w_lds"]), (le["an_lds"], le["c_lds"], le["a_lds"], le["w_lds"])) == want[name], (name, te, le)
    # the first event in frame order decides, as for the posteriors: from the restatements, on the smallest set
    streams, kinds = cases.event_batch()
    models = cases.event_models("5_3_4")
    lt = cases.event_prices(len(models))
    sym = np.concatenate(streams)
    offs = np.arange(len(streams) + 1, dtype=np.int64) * cases.EVENT_T
    status = [cases.event_status(k, "trans_posteriors") for k in kinds]
    assert status == [0] + [2] * 6 + [1] * 6 + [1, 2] * 3
    te = RTE.estep(models, sym, offs, lt)
    le = RLE.estep(models, sym, offs, lt, acc_trans=True)
    S = len(streams)
    for got in (te, le):
        assert got["status"].tolist() == status
        assert np.isfinite(got["log_prob"][0]) and (got["log_prob"][1:] == NINF).all()
    assert te["acc"][-2:].tolist() == [1, S - 1] == le["acc_trans"][-2:].tolist() and np.array_equal(te["acc"], le["acc_trans"])
    for (pi, _A, B), acc in zip(models, le["acc"]):
        lay = RLE.layout(len(pi), B.shape[1])
        assert (acc[lay["used"]], acc[lay["skipped"]]) == (1, S - 1)
    # a failed stream adds nothing: the limbs are the clean stream's alone
    alone = RLE.estep(models, streams[0], [0, cases.EVENT_T], lt, acc_trans=True)
    assert np.array_equal(alone["acc_trans"][:-2], le["acc_trans"][:-2]) and alone["acc_trans"][:-2].any()
    for (pi, _A, B), a, b in zip(models, alone["acc"], le["acc"]):
        used = RLE.layout(len(pi), B.shape[1])["used"]
        assert np.array_equal(a[:used], b[:used]) and a[:used].any()


@pytest.mark.parametrize("name", list(cases.GRAMMAR_SHAPES))
def test_the_grammar_session_restatement_delivers_frames_before_close_at_every_row(name):
    # (a GPU session test would else pass with every frame decided at close, the coalescence never having found a frame)
    _Ns, _M, T = cases.GRAMMAR_SHAPES[name]
    B = cases.SESSION_B
    rest, final_after = cases.trans_stream_reference(name)
    blocks = [final_after[p] for p in range(B, T + 1, B)]
    print(name, "final after each whole block:", blocks, "segments", sum(rest.entered), "classes", len(set(rest.cls)))
    assert rest.status == 0 and rest.join_failures == 0 and len(rest.cls) == T and len(blocks) == T // B >= 1
    assert 2 * sum(f > 0 for f in blocks) >= len(blocks)
    assert all(f <= p for f, p in zip(blocks, range(B, T + 1, B))) and blocks == sorted(blocks) and blocks[-1] > 0
    # the session is the one-shot decode of the restatement
    models, stream, lt = cases.grammar_shape(name)
    want = RT.segment_trans(models, stream, [0, T], lt)
    assert rest.cls == want["cls"].tolist() and rest.state == want["state"].tolist() and rest.entered == want["entered"].tolist()
    assert np.array_equal(_bits(np.array(rest.exit_score)), _bits(want["exit_score"]))
    assert _bits(rest.log_prob)[0] == _bits(want["log_prob"])[0] and want["entered"].sum() >= 8


# ---- what makes a row worth running ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.SHAPES))
def test_the_path_of_every_row_visits_many_classes_in_many_slots(name):
    Ns, _M, T = cases.SHAPES[name]
    want = cases.shape_reference(name)
    v = cases.visit(Ns, want["cls"], want["entered"])
    print(name, "segments", v["segments"], "classes", v["classes"], "slots", len(v["slots"]), "of", cases.slots_of(Ns))
    assert want["status"] == 0 and len(want["cls"]) == T and v["segments"] >= 10 and v["last_slot"]
    if name == "40_1x24_x14":
        # M = 4 there, and the classes that lean to one symbol differ only in how far: one of them takes every run of it.
        # The row is kept for its placement (lA beyond LDS with 25 classes to a slot), not for its path.
        assert v["classes"] >= 4
        return
    assert 2 * len(v["slots"]) >= cases.slots_of(Ns) or len(v["slots"]) >= 16
    # (composite indices beyond 3072 hold part of the path: the third and fourth state of a coalesce thread)
    if sum(Ns) == cases.SEG_MAX_SUM_N:
        comp0 = np.concatenate([[0], np.cumsum(Ns)])
        comp = comp0[want["cls"]] + want["state"]
        assert (comp >= 3 * cases.COALESCE_THREADS).any() and (comp >= 2 * cases.COALESCE_THREADS).sum() > T // 4


@pytest.mark.parametrize("name", cases.SESSION_SHAPES)
def test_a_session_over_the_row_decides_frames_after_every_block(name):
    _Ns, _M, T = cases.SHAPES[name]
    B = cases.SESSION_B
    rest, finals = cases.session_reference(name, "whole_blocks")
    print(name, "final after each block:", finals)
    assert rest.join_failures == 0 and rest.status == 0
    assert len(finals) == T // B + 1 and finals[0] > 0 and all(b > a for a, b in zip(finals, finals[1:T // B]))
    assert all(f <= (i + 1) * B for i, f in enumerate(finals))
    want = cases.shape_reference(name)
    assert rest.cls == want["cls"].tolist() and rest.state == want["state"].tolist() and rest.entered == want["entered"].tolist()
    assert np.array_equal(_bits(rest.gbest), _bits(want["gbest"])) and _bits(rest.log_prob)[0] == _bits(want["log_prob"])[0]
    if name == "64x64":  # live paths at composite indices above 3072 when the walk starts: d > -inf there after every block
        assert all((rest.ds[(i + 1) * B - 1][3 * cases.COALESCE_THREADS:] > NINF).any() for i in range(T // B))


# ---- the event streams -----------------------------------------------------------------------------------------------------------
def test_the_event_batch_is_the_one_the_align_tests_use():
    streams, kinds = cases.event_batch()
    assert len(streams) == 19 and kinds == ["clean"] + ["M"] * 6 + ["dead"] * 6 + ["dead_M", "M_dead"] * 3
    assert all(len(s) == cases.EVENT_T == 130 for s in streams) and cases.EVENT_EDGES == (0, 1, 63, 64, 65, 129)
    assert streams[0].max() < cases.DEAD < cases.EVENT_M == 8
    for s, p in zip(streams[1:7], cases.EVENT_EDGES):
        assert np.flatnonzero(s != streams[0]).tolist() == [p] and s[p] == cases.EVENT_M
    for s, p in zip(streams[7:13], cases.EVENT_EDGES):
        assert np.flatnonzero(s != streams[0]).tolist() == [p] and s[p] == cases.DEAD


@pytest.mark.parametrize("name", ["5_3_4", "64x17"])
def test_the_vectorised_restatements_are_their_literal_forms_on_the_event_streams(name):
    looped = name == "64x17"
    models = cases.event_models(name)
    streams, kinds = cases.event_batch()
    if looped:  # (the literal forms take a second a stream there: the clean one, one of each event, one pair of each order)
        keep = [0, 3, 9, 15, 16]
        streams, kinds = [streams[i] for i in keep], [kinds[i] for i in keep]
    lms = [V.log_model(*m) for m in models]
    lt = cases.event_prices(len(models))
    ls = cases.EVENT_LN_SWITCH
    for seq, kind in zip(streams, kinds):
        a = R.segment_logs(lms, seq, ls)
        c, s, e, G, lp, st = R.transcribe(models, seq, ls)
        assert (a["cls"].tolist(), a["state"].tolist(), a["entered"].tolist(), a["status"]) == (c, s, e, st), kind
        assert np.array_equal(_bits(a["gbest"]), _bits(G)) and _bits(a["log_prob"])[0] == _bits(lp)[0], kind
        assert st == cases.event_status(kind, "segment")
        a = RT.segment_trans_logs(lms, seq, lt)
        c, s, e, ex, lp, st = RT.transcribe(models, seq, lt)
        assert (a["cls"].tolist(), a["state"].tolist(), a["entered"].tolist(), a["status"]) == (c, s, e, st), kind
        assert np.array_equal(_bits(a["exit_score"]), _bits(ex)) and _bits(a["log_prob"])[0] == _bits(lp)[0], kind
        assert st == cases.event_status(kind, "trans")
        if looped:
            continue  # (17 slots: the posteriors refuse them)
        a = RP.posteriors_one(models, seq, ls)
        post, lp, st = RP.transcribe(models, seq, ls)
        assert np.array_equal(_bits(a["post"]), _bits(np.array(post).reshape(len(seq), len(models)))), kind
        assert _bits(a["log_prob"])[0] == _bits(lp)[0] and a["status"] == st == cases.event_status(kind, "posteriors"), kind
        if st != 0:
            assert not a["post"].any() and not np.signbit(a["post"]).any()


def test_the_status_of_every_event_stream_in_every_decoder():
    want = {"clean": (0, 0, 0, 0), "M": (2, 2, 2, 2), "dead": (1, 1, 1, 1), "M_dead": (2, 2, 2, 2), "dead_M": (2, 2, 1, 2)}
    for kind in cases.EVENT_KINDS:
        assert tuple(cases.event_status(kind, d) for d in ("segment", "trans", "posteriors", "stream")) == want[kind]
    # the session, whatever the feeds: the restatement's status at close
    lms = [V.log_model(*m) for m in cases.event_models()]
    streams, kinds = cases.event_batch()
    for seq, kind in zip(streams, kinds):
        for feeds in ([130], [64, 66], [1] * 130):
            log = cases.session_script(lms, seq, cases.EVENT_LN_SWITCH, cases.EVENT_SESSION_B, feeds)
            assert log[-1]["status"] == cases.event_status(kind, "stream"), (kind, feeds[0])
            assert log[-1]["final"] == log[-1]["fed"]  # (130, but for a feed that failed: what came after it was never given)


def test_what_the_session_restatement_does_with_a_bad_symbol_at_each_edge():
    lms = [V.log_model(*m) for m in cases.event_models()]
    clean = cases.event_batch()[0][0]
    B = cases.EVENT_SESSION_B
    assert B == 100 and cases.SESSION_BAD_AT == (0, 63, 64, 99, 100, 129)
    for p in cases.SESSION_BAD_AT:
        seq = cases.with_symbols(clean, {p: cases.EVENT_M})
        for feeds in ([130], [64, 66], [1] * 130):
            log = cases.session_script(lms, seq, cases.EVENT_LN_SWITCH, B, feeds)
            bad = [e for e in log if e.get("bad_frame") is not None]
            if p < B:  # the feed that completes the first block fails, with the frame in the error; nothing was final before
                assert len(bad) == 1 and bad[0]["bad_frame"] == p and bad[0]["final"] == 0, (p, feeds[0])
                assert bad[0]["fed"] == {1: 130, 2: 130, 130: B}[len(feeds)]  # (all of the failing feed counts as fed)
            else:  # the symbol waits in the remainder: no feed fails, and close meets it
                assert not bad and log[-2]["final"] > 0, (p, feeds[0])
            end = log[-1]
            fed = B if p < B and len(feeds) == 130 else 130  # (single symbols: the 100th feed fails, the rest is never given)
            assert (end["status"], end["log_prob"], end["final"], end["fed"]) == (2, NINF, fed, fed)
            n = fed - log[-2]["final"]
            assert end["out"]["cls"] == [0xFFFF] * n and end["out"]["gbest"] == [NINF] * n and end["out"]["entered"] == [0] * n


# ---- the random sets -------------------------------------------------------------------------------------------------------------
def test_the_random_sets_are_deterministic_and_meet_the_seed_rule():
    seed = cases.RANDOM_SEED
    assert cases.seed_rule(seed) and cases.first_seed(seed + 1) == seed == 4  # the first of 0, 1, 2, ... that meets the rule
    a, b = cases.random_sets(seed), cases.random_sets(seed)
    assert len(a) == 12
    for x, y in zip(a, b):
        assert x["Ns"] == y["Ns"] and x["M"] == y["M"] and _bits(x["ln_switch"])[0] == _bits(y["ln_switch"])[0]
        assert all(np.array_equal(s, t) for s, t in zip(x["streams"], y["streams"])) and len(x["streams"]) == 6
        assert all(np.array_equal(_bits(p), _bits(q)) for m, n in zip(x["models"], y["models"]) for p, q in zip(m, n))
        assert 1 <= len(x["Ns"]) <= 24 and set(x["Ns"]) <= set(cases.RANDOM_NS) and x["M"] in cases.RANDOM_MS
        assert x["ln_switch"] in cases.RANDOM_SWITCHES and all(len(s) <= 200 and (s < x["M"]).all() for s in x["streams"])
    slots = [cases.slots_of(x["Ns"]) for x in a]
    assert sum(s > 16 for s in slots) >= 3 and sum(cases.one_class_slot_next_to_packed(x["Ns"]) for x in a) >= 3
    res = cases.random_sets(seed, resident_only=True)
    assert len(res) == 12 and all(cases.slots_of(x["Ns"]) <= 16 for x in res)
    # the sets that were resident as drawn keep their classes
    assert all(x["Ns"] == y["Ns"] for x, y in zip(a, res) if cases.slots_of(x["Ns"]) <= 16)
    print("slots:", slots, "resident:", [cases.slots_of(x["Ns"]) for x in res], "M:", [x["M"] for x in a],
          "ln_switch:", [x["ln_switch"] for x in a])
