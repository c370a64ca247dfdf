"""what test_hmm_trans_fb_looped_cpu.py and test_gpu_hmm_trans_fb_looped.py share (TEST INFRASTRUCTURE): the looped bodies of
the two forward-backward passes under class-to-class prices -- `hmm segment --grammar-posteriors` (DESIGN.md 4.8.13,
hmm_posterior_trans_looped.hip) and the E-step of `hmm transitions --em` (4.8.14, hmm_trans_estep_looped.hip), both chosen by
ECOZ2_HMM_TRANS_FB_BODY -- the two restatements without their cap of 16 wave-slots, the class sets above 16 slots with their
models, streams, prices and references, what a reference has to show for a row to test anything, the event batches, the
planted training data, and the two LDS formulas restated."""
import contextlib
import functools

import numpy as np

from . import hmm_class_loop_cases as loop_cases
from . import hmm_trans_posterior_restatement as TP
from . import hmm_transitions_em_restatement as TE

NINF = float("-inf")
BODY = "ECOZ2_HMM_TRANS_FB_BODY"
OTHER_BODIES = ("ECOZ2_HMM_SEGMENT_TRANS_BODY", "ECOZ2_HMM_POSTERIOR_BODY")
CHUNK = "ECOZ2_HMM_POSTERIOR_CHUNK_BYTES"
ROUTE_C = "ECOZ2_HMM_TRANS_EM_C"
SEG_LDS_BYTES = loop_cases.SEG_LDS_BYTES
SEG_MAX_WAVES = loop_cases.SEG_MAX_WAVES
LENGTHS = (0, 1, 2, 63, 64, 65, 129)
MODEL_SEED, STREAM_SEED, PRICE_SEED = 7, 8, 3


# ---- the restatements at any number of slots -------------------------------------------------------------------------------------
@contextlib.contextmanager
def _uncapped():
    """posteriors_one and estep_one assert slots <= MAX_SLOTS, the resident bodies' limit, each on the name its own module
    imported; the global sum itself is defined for any number of slots"""
    before = TP.MAX_SLOTS, TE.MAX_SLOTS
    TP.MAX_SLOTS = TE.MAX_SLOTS = 1 << 30
    try:
        yield
    finally:
        TP.MAX_SLOTS, TE.MAX_SLOTS = before


def posteriors(models, sym, offs, lt):
    """hmm_trans_posterior_restatement.posteriors without the cap: the layout of ecoz2rs_amd.hmm.segment_trans_posteriors"""
    with _uncapped():
        return TP.posteriors(models, sym, offs, lt)


def estep(models, sym, offs, lt):
    """hmm_transitions_em_restatement.estep without the cap: the layout of ecoz2rs_amd.hmm.transitions_estep"""
    with _uncapped():
        return TE.estep(models, sym, offs, lt)


def train(models, sym, offs, **kw):
    with _uncapped():
        return TE.train(models, sym, offs, **kw)


# ---- class sets above 16 slots ---------------------------------------------------------------------------------------------------
# name: (N of every class, M) -- each over one stream per length of LENGTHS
WIDE = {
    "64x17": ((64,) * 17, 32),                   # 17 slots: wave 0 serves two; `single` chains; A global, w and C in LDS
    "33x17": ((33,) * 17, 8),                    # 17 slots; A (145 KB) still in LDS for the posteriors
    "33x20": ((33,) * 20, 32),                   # 20 slots, four waves with two turns
    "5x204": ((5,) * 204, 64),                   # 17 slots, twelve classes to a slot (ds_bpermute chains), K = 204; w and C global
    "8x136": ((8,) * 136, 16),                   # 17 slots of eight classes, K = 136: A in LDS next to global w and C
    "mixed_x9": ((3, 64, 7, 7, 33) * 9, 64),     # 19 slots, packed slots next to one-class slots
    "33x33": ((33,) * 33, 8),                    # 33 slots: three turns for wave 0, two for the rest
    "64x64": ((64,) * 64, 64),                   # 4096 states, four turns a wave
    "33x124": ((33,) * 124, 8),                  # 124 slots; A and w both global
}
SLOTS = {"64x17": 17, "33x17": 17, "33x20": 20, "5x204": 17, "8x136": 17, "mixed_x9": 19, "33x33": 33, "64x64": 64, "33x124": 124}
EVENT_ROWS = ("64x17", "33x20")
EVENT_T = 130
EVENT_AT = (0, 63, 64, 65, EVENT_T - 1)


def slots_of(Ns):
    return int(loop_cases.slot_of_class(Ns)[-1]) + 1


def a_words(Ns):
    return sum(N * (N | 1) for N in Ns)


def pack(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    sym = np.concatenate(seqs).astype(np.uint16) if seqs else np.zeros(0, np.uint16)
    return sym, offs


@functools.lru_cache(maxsize=None)
def wide_case(name):
    """-> (models, sym, offs, lt) of a row of WIDE (read only: the tests share it)"""
    Ns, M = WIDE[name]
    K = len(Ns)
    sym, offs = pack([loop_cases.run_stream(STREAM_SEED + i, K, M, T) for i, T in enumerate(LENGTHS)])
    return loop_cases.leaning_models(MODEL_SEED, Ns, M), sym, offs, loop_cases.forbidding_prices(PRICE_SEED, K)


@functools.lru_cache(maxsize=None)
def wide_posteriors(name):
    models, sym, offs, lt = wide_case(name)
    return posteriors(models, sym, offs, lt)


@functools.lru_cache(maxsize=None)
def wide_estep(name):
    models, sym, offs, lt = wide_case(name)
    return estep(models, sym, offs, lt)


def coverage(name):
    """what the two references of a row show -> dict: the largest posterior of a class in a slot >= 16 (a slot some wave serves
    in its second or a later turn) and of one in a slot < 16, and the cells of the count table with a non-zero limb from a slot
    < 16 into a slot >= 16 and back.  A row in which either side stays dark tests no looped body."""
    Ns, _M = WIDE[name]
    K = len(Ns)
    late = loop_cases.slot_of_class(Ns) >= SEG_MAX_WAVES
    post, acc = wide_posteriors(name)["post"], wide_estep(name)["acc"]
    cells = (acc[0:2 * K * K:2] != 0) | (acc[1:2 * K * K:2] != 0)
    cells = cells.reshape(K, K)
    return dict(post_late=float(post[:, late].max()), post_early=float(post[:, ~late].max()),
                into_late=int(cells[np.ix_(~late, late)].sum()), back_early=int(cells[np.ix_(late, ~late)].sum()))


# ---- events: a symbol outside the alphabet and a frame no state emits, between clean streams ---------------------------------------
@functools.lru_cache(maxsize=None)
def event_case(name):
    """-> (models, sym, offs, lt, kinds) of a row of EVENT_ROWS: the row's models with two symbols taken out -- DEAD = M - 1, which
    no state emits, and LATE = M - 2, which only the classes in a slot >= 16 emit.  Streams of EVENT_T frames: a clean one, then
    for p in EVENT_AT one with the symbol M at p and one that is LATE before p and DEAD at p (so the only live classes before the
    dead frame sit in a slot >= 16), a clean one in the middle and at the end.  kinds: "clean" / "M" / "dead" per stream."""
    Ns, M = WIDE[name]
    K = len(Ns)
    late = loop_cases.slot_of_class(Ns) >= SEG_MAX_WAVES
    DEAD, LATE = M - 1, M - 2
    models = []
    for k, (pi, A, B) in enumerate(loop_cases.leaning_models(MODEL_SEED, Ns, M)):
        B = B.copy()
        B[:, DEAD] = 0.0
        B[:, LATE] = 0.5 if late[k] else 0.0
        models.append((pi, A, B / B.sum(axis=1, keepdims=True)))
    clean = lambda i: (loop_cases.run_stream(STREAM_SEED + i, K, M - 2, EVENT_T) % (M - 2)).astype(np.uint16)
    streams, kinds = [clean(0)], ["clean"]
    for i, p in enumerate(EVENT_AT):
        if i == 2:
            streams.append(clean(1))
            kinds.append("clean")
        s = clean(2 + i)
        s[p] = M
        streams.append(s)
        kinds.append("M")
        s = clean(7 + i)
        s[:p] = LATE
        s[p] = DEAD
        streams.append(s)
        kinds.append("dead")
    streams.append(clean(12))
    kinds.append("clean")
    sym, offs = pack(streams)
    return models, sym, offs, loop_cases.forbidding_prices(PRICE_SEED, K), tuple(kinds)


@functools.lru_cache(maxsize=None)
def event_posteriors(name):
    models, sym, offs, lt, _kinds = event_case(name)
    return posteriors(models, sym, offs, lt)


@functools.lru_cache(maxsize=None)
def event_estep(name):
    models, sym, offs, lt, _kinds = event_case(name)
    return estep(models, sym, offs, lt)


# ---- a training on planted data ------------------------------------------------------------------------------------------------
TRAIN_ROW, TRAIN_ITERATIONS, TRAIN_STREAMS, TRAIN_T = "64x17", 3, 6, 96
TRAIN_KW = dict(ln_switch=-1.0, alpha=0.0, val_auto=-1e300, max_iterations=TRAIN_ITERATIONS)


@functools.lru_cache(maxsize=None)
def train_case():
    """-> (models, sym, offs) at TRAIN_ROW: streams that follow a planted grammar -- class k is followed by k + 1 (mod K) three
    times out of four, else by k + 5 --, eight frames a visit on the symbol the class leans to"""
    Ns, M = WIDE[TRAIN_ROW]
    K = len(Ns)
    rng = np.random.default_rng(11)
    streams = []
    for _ in range(TRAIN_STREAMS):
        k, out = int(rng.integers(0, K)), []
        while len(out) < TRAIN_T:
            out += [k % M] * 8
            k = (k + (1 if rng.random() < 0.75 else 5)) % K
        streams.append(np.array(out[:TRAIN_T], dtype=np.uint16))
    sym, offs = pack(streams)
    return loop_cases.leaning_models(MODEL_SEED, Ns, M), sym, offs


@functools.lru_cache(maxsize=None)
def train_reference():
    """the restatement's train over TRAIN_ITERATIONS E-steps (val_auto below any difference: no early stop; no smoothing, so
    that every M-step is Baum-Welch's own and L cannot fall)"""
    models, sym, offs = train_case()
    return train(models, sym, offs, **TRAIN_KW)


# ---- the LDS of the two looped bodies, restated; test_hmm_trans_fb_looped_cpu.py holds them against the sources -------------------
def posteriors_trans_looped_lds_bytes(slots, K, sumN, a_words_, a_lds, w_lds):
    """mandatory: the partial sums in both parities, the class masses of two steps, one double per composite state; A, then w
    with wT, behind them where they fit"""
    return (2 * slots + 2 * K + sumN + (a_words_ if a_lds else 0) + (2 * K * K if w_lds else 0)) * 8


def trans_estep_looped_lds_bytes(slots, K, sumN, a_words_, c_lds, a_lds, w_lds):
    """mandatory: the posteriors' terms and S_t per composite state; the C table, A, then w with wT, behind them"""
    return (2 * slots + 2 * K + 2 * sumN + (2 * K * K if c_lds else 0) + (a_words_ if a_lds else 0) + (2 * K * K if w_lds else 0)) * 8


def looped_route(Ns, c=None):
    """-> dict waves and, per pass, what its launcher decides: post = (a_lds, w_lds, bytes), estep = (c_lds, a_lds, w_lds,
    bytes); c: the route ECOZ2_HMM_TRANS_EM_C forces (True lds, False global)"""
    slots, K, sumN, aw = slots_of(Ns), len(Ns), sum(Ns), a_words(Ns)
    pl = lambda a, w: posteriors_trans_looped_lds_bytes(slots, K, sumN, aw, a, w)
    pa = pl(True, False) <= SEG_LDS_BYTES
    pw = pl(pa, True) <= SEG_LDS_BYTES
    el = lambda c_, a, w: trans_estep_looped_lds_bytes(slots, K, sumN, aw, c_, a, w)
    ec = el(True, False, False) <= SEG_LDS_BYTES if c is None else c
    ea = el(ec, True, False) <= SEG_LDS_BYTES
    ew = el(ec, ea, True) <= SEG_LDS_BYTES
    return dict(waves=min(slots, SEG_MAX_WAVES), post=(pa, pw, pl(pa, pw)), estep=(ec, ea, ew, el(ec, ea, ew)))


def most_mandatory_lds():
    """the largest mandatory LDS of the two passes over the class sets that segment_check_shape admits (N <= 64, K <= sum N <=
    4096): two neighbouring slots hold more than 64 states between them, so slots <= 2 * 4096 / 64 + 1 -- a bound no set
    reaches together with K = sum N = 4096, where the slots are 64"""
    n = loop_cases.SEG_MAX_SUM_N
    slots = 2 * n // 64 + 1
    return (posteriors_trans_looped_lds_bytes(slots, n, n, 0, False, False),
            trans_estep_looped_lds_bytes(slots, n, n, 0, False, False, False))
