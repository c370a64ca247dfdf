"""inputs that test_hmm_class_loop_cases_cpu.py, test_gpu_hmm_class_loop_shapes.py, test_gpu_hmm_trans_posteriors_shapes.py and
test_gpu_hmm_grammar_shapes.py share (TEST INFRASTRUCTURE): what the five class-loop decoders of DESIGN.md 4.8.6 - 4.8.9 and
4.8.13 (`hmm segment`, --posteriors, --class-transitions, --continuous, --grammar-posteriors), the two grammar trainers of
4.8.14 and 4.8.16 (`hmm transitions --em`, `hmm learn --loop`) and the grammar session of 4.8.15 (--grammar-continuous) are
run at beyond the tables of class sets of their own files -- streams with a bad or a dead symbol at the edges of the 64-symbol hand-out, class sets near the 4096 states the
decoders admit whose models lean so that the path visits many classes, the class sets that take --grammar-posteriors to each
of its four LDS layouts and above 64 KB of dynamic LDS, the class sets that take the trainers and the grammar session to each of theirs (GRAMMAR_SHAPES), and
seeded random sets -- and the LDS arithmetic of the eight launchers, restated."""
import functools

import numpy as np

from . import hmm_align_cases as align_cases
from . import hmm_segment_restatement as R
from . import hmm_loop_em_restatement as RLE
from . import hmm_segment_stream_restatement as RS
from . import hmm_segment_trans_stream_restatement as RTS
from . import hmm_trans_posterior_restatement as RTP
from . import hmm_transitions_em_restatement as RTE
from .hmm_align_cases import DEAD, EVENT_EDGES, EVENT_PAIRS_AT, EVENT_T, RANDOM_NS, slots_of  # noqa: F401  (for the tests as well)
from .hmm_segment_trans_cases import random_model, random_prices
from .hmm_viterbi_restatement import log_model

NINF = float("-inf")
EVENT_M = align_cases.M
EVENT_KINDS = ("clean", "M", "dead", "dead_M", "M_dead")
# the class sets the event streams are decoded under: one slot; six one-class slots, resident, whose lA (192 KB) stays in
# global memory; 17 slots, the first packing that is looped by itself (lA global as well)
EVENT_NS = {"5_3_4": (5, 3, 4), "64x6": (64,) * 6, "64x17": (64,) * 17,
            # --grammar-posteriors alone: pi, A and both price matrices above 64 KB of LDS; 14 slots of 25 classes, A and
            # the matrices in global memory, and 130 x 350 rows to zero behind an event
            "64x3": (64,) * 3, "40_1x24_x14": ((40,) + (1,) * 24) * 14}
# the event class sets of --grammar-posteriors, one per instantiation of k_hmm_loop_posteriors_trans<A_LDS, W_LDS>:
# <true, true>, <false, true>, <true, true> above 64 KB, <false, false>
TRANS_POSTERIORS_EVENT_SETS = ("5_3_4", "64x6", "64x3", "40_1x24_x14")
EVENT_LN_SWITCH = -0.5
EVENT_SESSION_B = 100  # frame 99 ends the block, 100 opens the remainder, 129 reaches the kernel only at close
SESSION_BAD_AT = (0, 63, 64, 99, 100, 129)
SESSION_DEAD_AT = (63, 64, 99, 100)


# ---- events at the edges of the 64-symbol hand-out -------------------------------------------------------------------------------
def event_models(name="5_3_4"):
    """dense models of EVENT_NS[name] no state of which emits DEAD"""
    return align_cases.event_models(EVENT_NS[name])


def event_batch():
    """-> (streams, kinds): hmm_align_cases.event_batch without its transcripts -- the clean stream; EVENT_M at p and DEAD at
    p for p in EVENT_EDGES; (DEAD, EVENT_M) and (EVENT_M, DEAD) at (a, a + 1) for a in EVENT_PAIRS_AT"""
    streams, _transcripts, _optionals, kinds = align_cases.event_batch()
    return streams, kinds


def event_status(kind, decoder):
    """the status of an event stream: any symbol >= M is 2 wherever it stands and a stream no path emits is 1 -- but the
    posteriors stop at the first event in frame order, so (DEAD, M) is 1 there"""
    if kind == "dead_M":
        return 1 if decoder in ("posteriors", "trans_posteriors") else 2
    return {"clean": 0, "M": 2, "dead": 1, "M_dead": 2}[kind]


def event_prices(K):
    """the prices the event batch is decoded under by --class-transitions"""
    return random_prices(np.random.default_rng(1), K)


def with_symbols(stream, at):
    out = np.array(stream, dtype=np.uint16)
    for t, o in at.items():
        out[t] = o
    return out


# ---- models that lean, streams that dwell ----------------------------------------------------------------------------------------
def leaning_models(seed, Ns, M, zeros=0.2):
    """random_model per class; class k then leans to the symbol k % M: without that, random models of many states give one
    segment in one class, and a session over them decides nothing before close"""
    rng = np.random.default_rng(seed)
    models = []
    for k, N in enumerate(Ns):
        pi, A, B = random_model(rng, N, M, zeros=zeros)
        B[:, k % M] *= rng.uniform(20, 60)
        models.append((pi, A, B / B.sum(axis=1, keepdims=True)))
    return models


def run_stream(seed, K, M, T, run=8):
    """runs of `run` frames, each on the symbol a class drawn uniformly from the K leans to"""
    rng = np.random.default_rng(seed)
    return (np.repeat(rng.integers(0, K, T // run + 1), run)[:T] % M).astype(np.uint16)


LN_SWITCH = -3.0
MODEL_SEED, STREAM_SEED = 7, 8
# name: (N of every class, M, T)
SHAPES = {
    "64x64": ([64] * 64, 64, 200),                      # 4096 states in 64 slots: four turns a looped wave, lA global, d > 64 KB
    "1x4096": ([1] * 4096, 64, 200),                    # 4096 classes in 64 full slots: lA in LDS next to d
    "1x1024": ([1] * 1024, 64, 130),                    # 16 full slots, resident: K = 1024 for segment and the posteriors
    "33x20": ([33] * 20, 32, 200),                      # looped, two slots to some waves
    "40_1x24_x14": (([40] + [1] * 24) * 14, 4, 130),    # 14 slots of 25 classes each: lA and lt global under the prices
}
SESSION_SHAPES = ("64x64", "33x20")
SESSION_B = 64


def shape(name):
    """-> (models, stream) of a row of SHAPES"""
    Ns, M, T = SHAPES[name]
    return leaning_models(MODEL_SEED, Ns, M), run_stream(STREAM_SEED, len(Ns), M, T)


@functools.lru_cache(maxsize=None)
def shape_reference(name):
    """hmm_segment_restatement.segment_logs of the row, computed once (read only: the tests share it)"""
    models, stream = shape(name)
    return R.segment_logs([log_model(*m) for m in models], stream, LN_SWITCH)


def session_feeds(T, pattern):
    """the feed lengths of `pattern`: "whole", "whole_blocks" (SESSION_B at a time) or "63_64_65" (in turn)"""
    if pattern == "whole":
        return [T]
    sizes = (SESSION_B,) if pattern == "whole_blocks" else (63, 64, 65)
    feeds = []
    while sum(feeds) < T:
        feeds.append(min(sizes[len(feeds) % len(sizes)], T - sum(feeds)))
    return feeds


@functools.lru_cache(maxsize=None)
def session_reference(name, pattern):
    """-> (the closed Stream of hmm_segment_stream_restatement, final frames after each feed) of the row at SESSION_B"""
    models, stream = shape(name)
    return RS.decode([log_model(*m) for m in models], stream, LN_SWITCH, SESSION_B, session_feeds(len(stream), pattern))


def forbidding_prices(seed, K, forbidden=0.2):
    """hmm_segment_trans_cases.random_prices from a seed: asymmetric prices in (-6, 0], a share of them -inf"""
    return random_prices(np.random.default_rng(seed), K, forbidden)


def session_script(lms, seq, ln_switch, B, feeds):
    """What a session does with the feeds, as hmm_segment_stream_restatement.Stream states it -> one entry per call, the
    last one for close: dict out (first, cls, state, entered, gbest of the frames the call made final; None where the feed
    failed), final (frames final after it), fed, bad_frame (of the feed that met a symbol outside the alphabet, else None);
    close adds status and log_prob.  After a feed has failed the session takes no more symbols: the script goes on to close."""
    s = RS.Stream(lms, ln_switch, B)
    log, at = [], 0
    for n in feeds:
        try:
            out, bad = s.feed(seq[at:at + n]), None
        except RS.BadSymbol as e:
            out, bad = None, e.frame
        at += n
        log.append(dict(out=out, final=s.F, fed=s.fed, bad_frame=bad))
        if bad is not None:
            break
    out = s.close()
    log.append(dict(out=out, final=s.F, fed=s.fed, bad_frame=None, status=s.status, log_prob=s.log_prob))
    return log


def slot_of_class(Ns):
    """the wave-slot of every class (pack_slots)"""
    out, slot, fill = [], -1, 64
    for N in Ns:
        if fill + N > 64:
            slot, fill = slot + 1, 0
        fill += N
        out.append(slot)
    return np.array(out, dtype=np.int64)


def visit(Ns, cls, entered):
    """what a decoded path makes of a class set -> dict segments, classes, slots (the set of slots the path is in), last_slot"""
    where = slot_of_class(Ns)
    used = set(int(k) for k in np.unique(cls))
    slots = set(int(where[k]) for k in used)
    return dict(segments=int(np.sum(entered)), classes=len(used), slots=slots, last_slot=int(where[-1]) in slots)


# ---- seeded random sets ----------------------------------------------------------------------------------------------------------
RANDOM_MS = (2, 8, 300)
RANDOM_SWITCHES = (NINF, -6.0, -3.0, -0.5, 0.0)
RANDOM_STREAMS = 6
RANDOM_MAX_K, RANDOM_MAX_T = 24, 200


ALONE_NS = tuple(N for N in RANDOM_NS if 2 * N > 64)  # 33, 40, 64: no two of them share a slot
ALONE_SHARES = (0.0, 0.5, 0.9)


def _class_sets(rng, n_sets):
    """K uniform in 1 .. 24 and K draws from RANDOM_NS per set.  Drawn uniformly, 24 classes take more than 16 slots once in
    ten thousand sets (measured on this draw), and no seed gives three such sets among twelve.  So every set first draws a share
    from ALONE_SHARES, and each of its N is with that chance one of ALONE_NS and else uniform over RANDOM_NS."""
    Ks = rng.integers(1, RANDOM_MAX_K + 1, n_sets)
    share = rng.choice(ALONE_SHARES, n_sets)
    Ns = np.where(rng.uniform(size=(n_sets, RANDOM_MAX_K)) < share[:, None], rng.choice(ALONE_NS, (n_sets, RANDOM_MAX_K)),
                  rng.choice(RANDOM_NS, (n_sets, RANDOM_MAX_K)))
    return [Ns[i, :Ks[i]].tolist() for i in range(n_sets)]


def random_shapes(seed, n_sets=12, resident_only=False):
    """the draw of random_sets before any model is built -> [dict Ns, M, ln_switch, model_seed, streams = [(T, runs, seed)]].
    Per set K uniform in 1 .. 24 and every N from RANDOM_NS (drawn again, with resident_only, while they take more than 16
    slots), M, ln_switch, and six streams of T uniform in 0 .. 200, each with equal chance a run_stream or uniform symbols."""
    rng = np.random.default_rng(seed)
    out = []
    for Ns in _class_sets(rng, n_sets):
        while resident_only and slots_of(Ns) > SEG_MAX_WAVES:
            Ns = _class_sets(rng, 1)[0]
        M = int(rng.choice(RANDOM_MS))
        ls = float(rng.choice(RANDOM_SWITCHES))
        model_seed = int(rng.integers(0, 2 ** 31))
        streams = [(int(rng.integers(0, RANDOM_MAX_T + 1)), bool(rng.integers(0, 2)), int(rng.integers(0, 2 ** 31)))
                   for _s in range(RANDOM_STREAMS)]
        out.append(dict(Ns=Ns, M=M, ln_switch=ls, model_seed=model_seed, streams=streams))
    return out


def random_sets(seed, n_sets=12, resident_only=False):
    """-> [dict Ns, M, ln_switch, models, streams]: random_shapes with its leaning models (zeros = 0.2) and its streams"""
    out = []
    for row in random_shapes(seed, n_sets, resident_only):
        K, M = len(row["Ns"]), row["M"]
        streams = [run_stream(s, K, M, T) if runs else np.random.default_rng(s).integers(0, M, T).astype(np.uint16)
                   for T, runs, s in row["streams"]]
        out.append(dict(Ns=row["Ns"], M=M, ln_switch=row["ln_switch"], models=leaning_models(row["model_seed"], row["Ns"], M),
                        streams=streams))
    return out


def one_class_slot_next_to_packed(Ns):
    """a slot that holds one class alone, and another that holds several: both kinds of in-class reads in one launch"""
    per_slot = np.bincount(slot_of_class(Ns))
    return bool((per_slot == 1).any() and (per_slot > 1).any())


def seed_rule(seed, n_sets=12):
    """what RANDOM_SEED has to meet, on the unrestricted draw: at least three sets of more than 16 slots (the looped body of
    `hmm segment` and of the session) and at least three with a one-class slot next to packed ones"""
    sets = _class_sets(np.random.default_rng(seed), n_sets)
    if sum(slots_of(Ns) > SEG_MAX_WAVES for Ns in sets) < 3:
        return False
    return sum(one_class_slot_next_to_packed(Ns) for Ns in sets) >= 3


def first_seed(limit):
    """the first of 0, 1, 2, ... below `limit` that meets seed_rule, or None"""
    return next((seed for seed in range(limit) if seed_rule(seed)), None)


# first_seed(): the first of 0, 1, 2, ... that meets seed_rule.  Chosen on the draw of the class sets alone, before any
# decoder ran on it: sets 1, 4 and 5 take 21, 22 and 21 slots, nine sets have a one-class slot next to packed ones.
RANDOM_SEED = 4


# ---- the LDS arithmetic of the eight launchers, restated; test_hmm_class_loop_cases_cpu.py holds it against the sources ----------
SEG_LDS_BYTES = align_cases.SEG_LDS_BYTES
SEG_MAX_WAVES = align_cases.SEG_MAX_WAVES
SEG_MAX_SUM_N = 4096
PAIR_BYTES = align_cases.PAIR_BYTES
LDS_OPT_IN = 64 * 1024  # above this a launcher has to raise the kernel's dynamic LDS limit first
COALESCE_THREADS = 1024
COALESCE_PER_THREAD = SEG_MAX_SUM_N // COALESCE_THREADS


def segment_lds_bytes(sumN, a_words, looped, a_lds):
    return 2 * SEG_MAX_WAVES * PAIR_BYTES + (a_words * 8 if a_lds else 0) + (2 * sumN * 8 if looped else 0)


stream_lds_bytes = segment_lds_bytes  # (the session's forward kernel has k_hmm_segment's layout)


def posteriors_lds_bytes(a_words, a_lds):
    return 2 * SEG_MAX_WAVES * 8 + (a_words * 8 if a_lds else 0)


def trans_lds_bytes(K, a_words, a_lds, lt_lds):
    return SEG_MAX_WAVES * PAIR_BYTES + 2 * K * 8 + (a_words * 8 if a_lds else 0) + (K * K * 8 if lt_lds else 0)


def trans_posteriors_lds_bytes(K, sumN, a_words, a_lds, w_lds):
    return (2 * SEG_MAX_WAVES + 2 * K + sumN + (a_words if a_lds else 0) + (2 * K * K if w_lds else 0)) * 8


def trans_estep_lds_bytes(K, sumN, a_words, c_lds, a_lds, w_lds):
    return (2 * SEG_MAX_WAVES + 2 * K + sumN + (2 * K * K if c_lds else 0) + (a_words if a_lds else 0) + (2 * K * K if w_lds else 0)) * 8


def loop_estep_lds_bytes(K, sumN, a_words, an_lds, c_lds, a_lds, w_lds):
    return (2 * SEG_MAX_WAVES + 2 * K + sumN + (2 * a_words if an_lds else 0) + (2 * K * K if c_lds else 0) +
            (a_words if a_lds else 0) + (2 * K * K if w_lds else 0)) * 8


def trans_stream_lds_bytes(K, a_words, a_lds, lt_lds):
    return 2 * K * 8 + (a_words * 8 if a_lds else 0) + (K * K * 8 if lt_lds else 0)


def route(decoder, Ns, looped=None, gram=True, an=None, c=None):
    """-> dict body ("resident" / "looped"), a_lds, lt_lds (trans and trans_stream alone; else None), lds: what the launcher of
    `decoder` ("segment", "stream", "posteriors", "trans", "trans_posteriors", "trans_estep", "loop_estep" or "trans_stream")
    decides for the class set; looped: ECOZ2_HMM_SEGMENT_BODY=looped.  "trans_posteriors" adds w_lds: both price matrices of
    4.8.13, placed after A.  The two trainers (4.8.14, 4.8.16) add c_lds, the count table of the grammar, and "loop_estep"
    an_lds, the AN table over all classes, before it; gram: the call forms the grammar counts (else c_lds is None); an / c:
    the route ECOZ2_HMM_LOOP_EM_AN / ECOZ2_HMM_LOOP_EM_C (for "trans_estep" ECOZ2_HMM_TRANS_EM_C) forces, True for lds, False
    for global.  A forced route may ask for more than SEG_LDS_BYTES: the host refuses that call."""
    slots, sumN, K = slots_of(Ns), sum(Ns), len(Ns)
    if decoder in ("segment", "stream"):
        if looped is None:
            looped = False
        looped = looped or slots > SEG_MAX_WAVES
        a_words = sum(N * N for N in Ns)
        a_lds = segment_lds_bytes(sumN, a_words, looped, True) <= SEG_LDS_BYTES
        return dict(body="looped" if looped else "resident", a_lds=a_lds, lt_lds=None,
                    lds=segment_lds_bytes(sumN, a_words, looped, a_lds))
    assert slots <= SEG_MAX_WAVES and not looped, "only the resident layout exists"
    if decoder == "posteriors":
        a_words = sum(N * (N | 1) for N in Ns)  # (the leading dimension is odd there)
        a_lds = posteriors_lds_bytes(a_words, True) <= SEG_LDS_BYTES
        return dict(body="resident", a_lds=a_lds, lt_lds=None, lds=posteriors_lds_bytes(a_words, a_lds))
    if decoder == "trans_posteriors":
        a_words = sum(N * (N | 1) for N in Ns)  # (posteriors_a_ld)
        a_lds = trans_posteriors_lds_bytes(K, sumN, a_words, True, False) <= SEG_LDS_BYTES
        w_lds = trans_posteriors_lds_bytes(K, sumN, a_words, a_lds, True) <= SEG_LDS_BYTES
        return dict(body="resident", a_lds=a_lds, lt_lds=None, w_lds=w_lds,
                    lds=trans_posteriors_lds_bytes(K, sumN, a_words, a_lds, w_lds))
    if decoder == "trans_estep":  # the decision order: c, a, w
        a_words = sum(N * (N | 1) for N in Ns)  # (posteriors_a_ld)
        lds = lambda *where: trans_estep_lds_bytes(K, sumN, a_words, *where)
        c_lds = lds(True, False, False) <= SEG_LDS_BYTES if c is None else c
        a_lds = lds(c_lds, True, False) <= SEG_LDS_BYTES
        w_lds = lds(c_lds, a_lds, True) <= SEG_LDS_BYTES
        return dict(body="resident", c_lds=c_lds, a_lds=a_lds, lt_lds=None, w_lds=w_lds, lds=lds(c_lds, a_lds, w_lds))
    if decoder == "loop_estep":  # the decision order: an, c (with the grammar table alone), a, w
        a_words = sum(N * (N | 1) for N in Ns)  # (posteriors_a_ld)
        lds = lambda *where: loop_estep_lds_bytes(K, sumN, a_words, *where)
        an_lds = lds(True, False, False, False) <= SEG_LDS_BYTES if an is None else an
        if not gram:
            c_lds = False
        else:
            c_lds = lds(an_lds, True, False, False) <= SEG_LDS_BYTES if c is None else c
        a_lds = lds(an_lds, c_lds, True, False) <= SEG_LDS_BYTES
        w_lds = lds(an_lds, c_lds, a_lds, True) <= SEG_LDS_BYTES
        return dict(body="resident", an_lds=an_lds, c_lds=c_lds if gram else None, a_lds=a_lds, lt_lds=None, w_lds=w_lds,
                    lds=lds(an_lds, c_lds, a_lds, w_lds))
    assert decoder in ("trans", "trans_stream")
    a_words = sum(N * N for N in Ns)
    a_lds = trans_lds_bytes(K, a_words, True, False) <= SEG_LDS_BYTES
    lt_lds = trans_lds_bytes(K, a_words, a_lds, True) <= SEG_LDS_BYTES
    if decoder == "trans_stream":  # segment_trans_layout's decision; the session's kernel is launched without the pairs
        return dict(body="resident", a_lds=a_lds, lt_lds=lt_lds, lds=trans_stream_lds_bytes(K, a_words, a_lds, lt_lds))
    return dict(body="resident", a_lds=a_lds, lt_lds=lt_lds, lds=trans_lds_bytes(K, a_words, a_lds, lt_lds))


# ---- --grammar-posteriors (4.8.13) at every LDS layout ---------------------------------------------------------------------------
TRANS_POSTERIORS_T = 130
TRANS_POSTERIORS_PRICE_SEED = 3
# name: (N of every class, M): leaning models, a dwelling stream of TRANS_POSTERIORS_T frames, forbidding_prices(3, K).
# Behind each row: the instantiation of k_hmm_loop_posteriors_trans<A_LDS, W_LDS> and the dynamic LDS it is launched with
# (test_hmm_class_loop_cases_cpu.py asserts both through route()).
TRANS_POSTERIORS_SHAPES = {
    "64x3": ([64] * 3, 64),                           # <true, true>, 101,824 B: the opt-in above 64 KB
    "64x6_1x84": ([64] * 6 + [1] * 84, 64),           # <false, true>, 135,040 B: the opt-in; K = 90 in 8 slots
    "40_1x24_x6": (([40] + [1] * 24) * 6, 4),         # <true, false>, 85,600 B: the opt-in; K = 150 in 6 slots
    "64x4_1x768": ([64] * 4 + [1] * 768, 64),         # <true, false>, 160,064 B: 3,776 B under the cap; K = 772 in 16 slots
    "1x1024": ([1] * 1024, 64),                       # <true, false>, 33,024 B: the most classes admitted, 16 full slots
    "40_1x24_x14": (([40] + [1] * 24) * 14, 4),       # <false, false>, 13,024 B: K = 350, 25 classes to a slot
    "64x8_1x512": ([64] * 8 + [1] * 512, 64),         # <false, false>, 16,768 B: eight one-class slots (the readlane chains)
}


def trans_posteriors_shape(name):
    """-> (models, stream, lt) of a row of TRANS_POSTERIORS_SHAPES"""
    Ns, M = TRANS_POSTERIORS_SHAPES[name]
    K = len(Ns)
    return (leaning_models(MODEL_SEED, Ns, M), run_stream(STREAM_SEED, K, M, TRANS_POSTERIORS_T),
            forbidding_prices(TRANS_POSTERIORS_PRICE_SEED, K))


@functools.lru_cache(maxsize=None)
def trans_posteriors_reference(name):
    """hmm_trans_posterior_restatement.posteriors of the row, computed once (read only: the tests share it)"""
    models, stream, lt = trans_posteriors_shape(name)
    return RTP.posteriors(models, stream, [0, len(stream)], lt)


@functools.lru_cache(maxsize=None)
def trans_posteriors_event_reference(name):
    """the restatement of the event batch under event_models(name) and event_prices(K), computed once (read only)"""
    streams, _kinds = event_batch()
    models = event_models(name)
    sym = np.concatenate(streams)
    offs = np.arange(len(streams) + 1, dtype=np.int64) * EVENT_T
    return RTP.posteriors(models, sym, offs, event_prices(len(models)))


# ---- the grammar trainers and the grammar session (4.8.14 - 4.8.16) at every LDS layout ------------------------------------------
# name: (N of every class, M, T): the rows of TRANS_POSTERIORS_SHAPES and six more, built as those are -- leaning models, a
# dwelling stream of T frames, forbidding_prices(3, K).  Behind each row what the three launchers make of it (asserted through
# route() in test_hmm_class_loop_cases_cpu.py): k_hmm_trans_estep's (c, a, w) and bytes | k_hmm_loop_estep's (an, c, a, w) and
# bytes with the grammar table | k_hmm_segment_trans_stream's (a, lt) and bytes.  T / F: in LDS / in global memory.
GRAMMAR_SHAPES = {
    "64x3": ([64] * 3, 64, 130),                          # TTT 101,968 | FTTT 101,968 | TT 98,424
    "64x6_1x84": ([64] * 6 + [1] * 84, 64, 130),          # TFF 135,040 | FTFF 135,040; without the table F-FT | FT 66,240
    "40_1x24_x6": (([40] + [1] * 24) * 6, 4, 130),        # FTF 85,600 | FFTF 85,600 | TF 80,352
    "64x4_1x768": ([64] * 4 + [1] * 768, 64, 130),        # FTF 160,064 | FFTF 160,064 | TF 149,568
    # (the C table in global memory at K = 1024, about 10^6 limb pairs a frame: 605 ms and 599 ms of kernel time for the 130
    # frames in the two trainers on one MI355X, so T stays 130)
    "1x1024": ([1] * 1024, 64, 130),                      # FTF 33,024 | TFTF 49,408 | TF 24,576
    "40_1x24_x14": (([40] + [1] * 24) * 14, 4, 130),      # FFF 13,024 | FFFF 13,024 | FF 5,600
    "64x8_1x512": ([64] * 8 + [1] * 512, 64, 130),        # FFF 16,768 | FFFF 16,768 | FF 8,320
    "64x2": ([64] * 2, 64, 130),                          # TTT 68,000 | TTFT 134,560: AN in LDS, A global | TT 65,600
    "1x71": ([1] * 71, 64, 130),                          # TTT 163,840: the cap exactly | TTTF 84,320 | TT 42,032
    "1x80": ([1] * 80, 64, 130),                          # TTF 105,216 | TTTF 106,496 | TT 53,120
    "64_1x64": ([64] + [1] * 64, 64, 130),                # TTF 103,712 | TTFF 137,504 | TT 68,120
    "64x2_1x60": ([64] * 2 + [1] * 60, 64, 130),          # TTF 131,296 | TFFF 136,832 | TT 97,760
    "64x3_1x64": ([64] * 3 + [1] * 64, 64, 130),          # TFT 147,024 | FTFT 147,024; without the table F-TF 103,728 | TT 135,800
}
GRAMMAR_EVENT_SETS = TRANS_POSTERIORS_EVENT_SETS + ("64x2",)  # (AN in LDS next to A in global memory, an event behind it)
EVENT_NS["64x2"] = (64,) * 2


def grammar_shape(name):
    """-> (models, stream, lt) of a row of GRAMMAR_SHAPES"""
    Ns, M, T = GRAMMAR_SHAPES[name]
    K = len(Ns)
    return leaning_models(MODEL_SEED, Ns, M), run_stream(STREAM_SEED, K, M, T), forbidding_prices(TRANS_POSTERIORS_PRICE_SEED, K)


@functools.lru_cache(maxsize=None)
def trans_estep_reference(name):
    """hmm_transitions_em_restatement.estep of the row, computed once (read only: the tests share it)"""
    models, stream, lt = grammar_shape(name)
    return RTE.estep(models, stream, [0, len(stream)], lt)


@functools.lru_cache(maxsize=None)
def loop_estep_reference(name):
    """hmm_loop_em_restatement.estep of the row with the grammar table, computed once (read only)"""
    models, stream, lt = grammar_shape(name)
    return RLE.estep(models, stream, [0, len(stream)], lt, acc_trans=True)


@functools.lru_cache(maxsize=None)
def trans_stream_reference(name):
    """-> (the closed Stream of hmm_segment_trans_stream_restatement at SESSION_B, fed whole; final_after(p) at every multiple p
    of SESSION_B: the frames a session has delivered once it has processed p of them, whatever the feeds), computed once"""
    models, stream, lt = grammar_shape(name)
    rest, _finals = RTS.decode([log_model(*m) for m in models], stream, lt, SESSION_B, [len(stream)])
    return rest, {p: rest.final_after(p) for p in range(0, len(stream) + 1, SESSION_B)}


@functools.lru_cache(maxsize=None)
def grammar_event_reference(name):
    """-> (hmm_transitions_em_restatement.estep, hmm_loop_em_restatement.estep with the grammar table) of the clean stream of the
    event batch alone, under event_models(name) and event_prices(K), computed once (read only): a failed stream adds nothing
    but its mark, so these are the limbs of the whole batch"""
    streams, _kinds = event_batch()
    models = event_models(name)
    lt = event_prices(len(models))
    return RTE.estep(models, streams[0], [0, EVENT_T], lt), RLE.estep(models, streams[0], [0, EVENT_T], lt, acc_trans=True)
