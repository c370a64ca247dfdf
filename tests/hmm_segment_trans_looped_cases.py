"""what test_hmm_segment_trans_looped_cpu.py and test_gpu_hmm_segment_trans_looped.py share (TEST INFRASTRUCTURE): the looped
body of `hmm segment --class-transitions` and of its session (ECOZ2_HMM_SEGMENT_TRANS_BODY,
hmm_segment_trans_looped.hip) -- the class sets above 16 wave-slots with their models, streams, prices and references, what a
decoded path has to visit for a row to test anything, and the LDS formula restated."""
import functools

import numpy as np

from . import hmm_class_loop_cases as loop_cases
from . import hmm_segment_trans_restatement as RT
from . import hmm_segment_trans_stream_restatement as ST
from .hmm_viterbi_restatement import log_model

NINF = float("-inf")
BODY = "ECOZ2_HMM_SEGMENT_TRANS_BODY"
CHUNK = "ECOZ2_HMM_SEGMENT_CHUNK_BYTES"
ENV_BLOCK = "ECOZ2_HMM_SEGMENT_STREAM_BLOCK"
ENV_PENDING = "ECOZ2_HMM_SEGMENT_STREAM_PENDING_BYTES"
SEG_LDS_BYTES = loop_cases.SEG_LDS_BYTES
SEG_MAX_WAVES = loop_cases.SEG_MAX_WAVES
PAIR_BYTES = loop_cases.PAIR_BYTES
MODEL_SEED, STREAM_SEED, PRICE_SEED = 7, 8, 3
SESSION_B = loop_cases.SESSION_B
KEYS = ("cls", "state", "entered", "exit_score", "log_prob", "status")

# name: (N of every class, M, T) -- the smallest shapes at which the looped body can still go wrong
WIDE = {
    "64x17": ((64,) * 17, 32, 200),                       # 17 slots: wave 0 serves two, the others one; the `single` route
    "33x20": ((33,) * 20, 32, 200),                       # 20 slots, four waves with two turns
    "5x204": ((5,) * 204, 64, 200),                       # 17 packed slots of 12 classes, 4 idle lanes each; K = 204
    "mixed_x9": ((3, 64, 7, 7, 33) * 9, 64, 200),         # 19 slots, packed slots next to one-class slots
    "1x1088": ((1,) * 1088, 64, 130),                     # 17 full slots, K = 1088: lt (9.5 MB) global, A in LDS
    "40_1x24_x18": (((40,) + (1,) * 24) * 18, 4, 130),    # 18 slots of 25 classes each
    "64x64": ((64,) * 64, 64, 200),                       # 4096 states, four turns a wave, A global, the largest carry arrays
}
SESSION_ROWS = ("64x17", "33x20", "64x64")
# the rows of test_gpu_hmm_segment_trans.py at which the looped body is forced below the cap (one per (A, lt) placement among them)
BELOW_THE_CAP = ("1", "handout", "5x12", "40_40", "mixed", "64x16", "1x1024", "40_1x24_x14")


def slots_of(Ns):
    return int(loop_cases.slot_of_class(Ns)[-1]) + 1


@functools.lru_cache(maxsize=None)
def wide_case(name):
    """-> (models, stream, lt) of a row of WIDE (read only: the tests share it)"""
    Ns, M, T = WIDE[name]
    K = len(Ns)
    return (loop_cases.leaning_models(MODEL_SEED, Ns, M), loop_cases.run_stream(STREAM_SEED, K, M, T),
            loop_cases.forbidding_prices(PRICE_SEED, K))


@functools.lru_cache(maxsize=None)
def wide_reference(name):
    """hmm_segment_trans_restatement.segment_trans of the row, computed once (read only)"""
    models, stream, lt = wide_case(name)
    return RT.segment_trans(models, stream, np.array([0, len(stream)], dtype=np.int64), lt)


@functools.lru_cache(maxsize=None)
def session_reference(name, pattern):
    """-> (the closed Stream of hmm_segment_trans_stream_restatement at SESSION_B, final frames after each feed) of the row"""
    models, stream, lt = wide_case(name)
    return ST.decode([log_model(*m) for m in models], stream, lt, SESSION_B, loop_cases.session_feeds(len(stream), pattern))


def crossings(Ns, ref):
    """what the decoded path of a one-stream reference makes of the class set -> dict status, slots, into_late (entries into a
    class in a slot >= 16: a slot some wave serves in its second or a later turn), back_early (entries into a slot < 16 that
    leave a class in a slot >= 16).  A row whose path never crosses between the turns in both directions tests no looped body."""
    where = loop_cases.slot_of_class(Ns)
    cls, entered = ref["cls"], ref["entered"]
    into_late = back_early = 0
    for t in np.flatnonzero(entered):
        if t == 0:
            continue
        to, frm = int(where[cls[t]]), int(where[cls[t - 1]])
        into_late += to >= SEG_MAX_WAVES
        back_early += to < SEG_MAX_WAVES <= frm
    return dict(status=int(ref["status"][0]), slots=slots_of(Ns), segments=int(np.sum(entered)), into_late=int(into_late),
                back_early=int(back_early))


# ---- the LDS of the looped body, restated; test_hmm_segment_trans_looped_cpu.py holds it against the source ---------------------
def segment_trans_looped_lds_bytes(K, sumN, a_words, a_lds, lt_lds):
    """mandatory: the pairs of the last maximum, E of two frames, and per composite state d and best (doubles) and arg (int);
    A, and then ltT, behind them where they fit"""
    return SEG_MAX_WAVES * PAIR_BYTES + 2 * K * 8 + sumN * (8 + 8 + 4) + (a_words * 8 if a_lds else 0) + (K * K * 8 if lt_lds else 0)


def looped_route(Ns):
    """-> dict waves, a_lds, lt_lds, lds: what the two looped launchers decide for the class set"""
    K, sumN, aw = len(Ns), sum(Ns), sum(N * N for N in Ns)
    lds = lambda a, l: segment_trans_looped_lds_bytes(K, sumN, aw, a, l)
    a_lds = lds(True, False) <= SEG_LDS_BYTES
    lt_lds = lds(a_lds, True) <= SEG_LDS_BYTES
    return dict(waves=min(slots_of(Ns), SEG_MAX_WAVES), a_lds=a_lds, lt_lds=lt_lds, lds=lds(a_lds, lt_lds))


def most_mandatory_lds():
    """the largest mandatory LDS a class set that segment_check_shape admits (K <= sum N <= 4096) can ask for"""
    n = loop_cases.SEG_MAX_SUM_N
    return segment_trans_looped_lds_bytes(n, n, 0, False, False)
