"""inputs that test_hmm_align_cpu.py and test_gpu_hmm_align.py share (TEST INFRASTRUCTURE): the packings, transcripts and
streams of DESIGN.md 4.8.10, and the planted stream -- sampled from three small left-to-right models in a known order with an
optional filler between them -- whose true boundaries the alignment has to find."""
import numpy as np

from .hmm_segment_trans_cases import random_model

NINF = float("-inf")
M = 8

# name: (N of every model, the transcript as model indices -- each contains an immediate repeat --, stream length)
PACKINGS = {
    "5x13": ([5, 5, 5], [0, 1, 2, 0, 0, 1, 2, 0, 1, 2, 0, 1, 2], 400),             # two packed slots
    "mixed": ([3, 64, 7, 33], [0, 1, 2, 2, 3], 400),                                # packed next to one-unit slots
    "64x16": ([64, 64, 64], [0, 1, 2, 2] * 4, 400),                                 # 16 slots: the widest resident shape
    "64x17": ([64, 64, 64], [0, 1, 2, 2] * 4 + [1], 400),                           # the first looped shape
    "33x20": ([33, 33, 33, 33, 33], [0, 1, 2, 3, 4, 4, 3, 2, 1, 0] * 2, 400),       # looped: two slots to some waves
}


def packing(name):
    """-> (models, units, stream): models with zeros in pi and A (-inf occurs), a stream that dwells on runs of symbols"""
    Ns, units, T = PACKINGS[name]
    rng = np.random.default_rng(sum(Ns) + len(units))
    models = [random_model(rng, N, M, zeros=0.3) for N in Ns]
    runs = rng.integers(0, M, T // 4 + 1)
    stream = np.where(rng.uniform(size=T) < 0.7, np.repeat(runs, 4)[:T], rng.integers(0, M, T)).astype(np.uint16)
    return models, np.array(units, dtype=np.int32), stream


# ---- the shapes where classes and units part: A is sized by the classes, slots / L / sum N by the transcript --------------------
# name: (N of every model, transcript, optional units or None, stream length, M, zeros, {frame: symbol} set after the draw).
# Next to PACKINGS and not in it: only the GPU files (test_gpu_hmm_*_shapes.py) run these.
_CYCLE17 = [l % 6 for l in range(17)]
_CYCLE17[9] = _CYCLE17[8]  # (one immediate repeat)
SHAPES = {
    "64x6c_8u": ([64] * 6, [0, 1, 2, 3, 4, 5, 5, 0], None, 100, 8, 0.3, {}),         # lA of the classes = 192 KB, 8 slots
    "64x6c_17u": ([64] * 6, _CYCLE17, None, 100, 8, 0.3, {}),                         # the same classes, 17 slots
    "21x48c": ([21] * 48, list(range(48)), None, 120, 8, 0.3, {}),                    # lA = 165 KB, three units to a wave, 16 slots
    "1x3c_200u": ([1, 1, 1], [l % 3 for l in range(200)], None, 260, 8, 0.3, {}),     # 64 units to a slot, the last slot 8 lanes
    "1x3c_201u_opt": ([1, 1, 1], [l % 3 for l in range(201)], list(range(0, 201, 2)), 150, 8, 0.0, {}),  # T < L
    "1_64_1": ([1, 64], [0] * 70 + [1] + [0] * 70, None, 200, 8, 0.3, {}),            # one-state slots around a one-unit slot
    "mixed_M1024": ([3, 64, 7, 33], [0, 1, 2, 2, 3], None, 400, 1024, 0.3, {}),
    "small_M65536": ([3, 4], [0, 1, 0], None, 70, 65536, 0.3, {10: 65535, 64: 65535}),  # the top symbol is legal
}
# the rows whose lA does not fit LDS next to the rest, with the body of k_hmm_align that decodes them
A_GLOBAL = {"64x6c_8u": "resident", "64x6c_17u": "looped", "21x48c": "resident"}


def shape(name, seed=None):
    """-> (models, units, optional or None, stream) of a row of SHAPES; `seed`: another draw of the stream under the same models"""
    Ns, units, opt, T, m, zeros, planted_syms = SHAPES[name]
    rng = np.random.default_rng(sum(Ns) + len(units))
    models = [random_model(rng, N, m, zeros=zeros) for N in Ns]
    if seed is not None:
        rng = np.random.default_rng(seed)
    runs = rng.integers(0, m, T // 4 + 1)
    stream = np.where(rng.uniform(size=T) < 0.7, np.repeat(runs, 4)[:T], rng.integers(0, m, T)).astype(np.uint16)
    for t, o in planted_syms.items():
        stream[t] = o
    optional = None
    if opt is not None:
        optional = np.zeros(len(units), np.uint8)
        optional[opt] = 1
    return models, np.array(units, dtype=np.int32), optional, stream


# the LDS arithmetic of hmm_align.hip and hmm_embed.hip, restated; test_hmm_align_cpu.py holds the constants against the headers
SEG_LDS_BYTES = 160 * 1024
SEG_MAX_WAVES = 16
PAIR_BYTES = 16


def slots_of(uN):
    """the wave-slots of 64 lanes that units of uN states take, packed in order (pack_slots)"""
    slots, fill = 0, 64
    for N in uN:
        if fill + N > 64:
            slots, fill = slots + 1, 0
        fill += N
    return slots


def align_lds_bytes(max_L, max_sumN, a_words, looped, a_lds):
    return SEG_MAX_WAVES * PAIR_BYTES + 2 * max_L * 8 + (a_words * 8 if a_lds else 0) + (2 * max_sumN * 8 if looped else 0)


def embed_lds_bytes(max_L, a_words, a_lds, an_lds):
    return 2 * SEG_MAX_WAVES * 8 + 2 * max_L * 8 + (a_words * 8 if a_lds else 0) + (a_words * 16 if an_lds else 0)


def align_route(Ns, units, looped=None):
    """-> (looped, a_lds) as align_plan and launch_align decide them for one stream in a launch of its own"""
    uN = [Ns[k] for k in units]
    if looped is None:
        looped = slots_of(uN) > SEG_MAX_WAVES
    a_words = sum(N * N for N in Ns)
    return looped, align_lds_bytes(len(uN), sum(uN), a_words, looped, True) <= SEG_LDS_BYTES


def embed_route(Ns, max_L):
    """-> (a_lds, an_lds) as embed_plan decides them with neither forced; A has the leading dimension N | 1 there"""
    a_words = sum(N * (N | 1) for N in Ns)
    a_lds = embed_lds_bytes(max_L, a_words, True, False) <= SEG_LDS_BYTES
    return a_lds, embed_lds_bytes(max_L, a_words, a_lds, True) <= SEG_LDS_BYTES


# ---- events at the edges of the 64-symbol hand-out -------------------------------------------------------------------------------
EVENT_T = 130
EVENT_EDGES = (0, 1, 63, 64, 65, EVENT_T - 1)
EVENT_PAIRS_AT = (0, 63, 64)
DEAD = 5  # the symbol no state emits


def event_models(Ns=(5, 3, 4)):
    """dense models (three by default) whose states cannot emit DEAD"""
    out = []
    for pi, A, B in small_models(seed=3, Ns=Ns, zeros=0.0):
        B = B.copy()
        B[:, DEAD] = 0.0
        out.append((pi, A, B / B.sum(axis=1, keepdims=True)))
    return out


def event_batch():
    """-> (streams, transcripts, optionals, kinds): the clean stream; M at p and DEAD at p for the edges p; (DEAD, M) and
    (M, DEAD) at (a, a + 1).  kinds[s]: "clean", "M", "dead", "dead_M" or "M_dead" """
    rng = np.random.default_rng(130)
    clean = rng.integers(0, DEAD, EVENT_T).astype(np.uint16)
    streams, kinds = [clean], ["clean"]

    def add(kind, at):
        s = clean.copy()
        for t, o in at.items():
            s[t] = o
        streams.append(s)
        kinds.append(kind)

    for p in EVENT_EDGES:
        add("M", {p: M})
    for p in EVENT_EDGES:
        add("dead", {p: DEAD})
    for a in EVENT_PAIRS_AT:
        add("dead_M", {a: DEAD, a + 1: M})
        add("M_dead", {a: M, a + 1: DEAD})
    n = len(streams)
    return streams, [np.array([0, 1, 2, 1], np.int32)] * n, [np.array([0, 1, 0, 0], np.uint8)] * n, kinds


# ---- a resident launch of unlike streams -----------------------------------------------------------------------------------------
def unlike_streams():
    """-> (models, streams, transcripts, optionals): four streams of 1, 2, 8 and 3 slots over classes 0 .. 2 of N = 5 ("5x13")
    and 3 .. 5 of N = 64 (the first three of "64x6c_8u")"""
    models = packing("5x13")[0] + shape("64x6c_8u")[0][:3]
    rng = np.random.default_rng(77)
    streams = [rng.integers(0, M, n).astype(np.uint16) for n in (5, 64, 129, 65)]
    transcripts = [np.array([1], np.int32), np.array(PACKINGS["5x13"][1], np.int32),
                   np.array([3 + k % 3 for k in SHAPES["64x6c_8u"][1]], np.int32), np.array([l % 3 for l in range(30)], np.int32)]
    optionals = [np.zeros(len(u), np.uint8) for u in transcripts]
    optionals[1][[0, 4, 12]] = 1
    optionals[2][[1, 6]] = 1
    optionals[3][1::2] = 1
    return models, streams, transcripts, optionals


# ---- a seeded random batch -------------------------------------------------------------------------------------------------------
RANDOM_NS = (1, 2, 3, 5, 8, 13, 21, 33, 40, 64)


def random_batch(seed, max_L, max_slots=None, S=40):
    """-> (models, streams, transcripts, optionals): ten models of RANDOM_NS (zeros = 0.2); per stream L uniform in 1 .. max_L,
    the units uniform over the models (drawn again while they take more than max_slots slots), a unit optional with
    probability 0.3 unless the one before is, never all of them; T uniform in max(1, L - 2) .. L + 150"""
    rng = np.random.default_rng(seed)
    models = [random_model(rng, N, M, zeros=0.2) for N in RANDOM_NS]
    streams, transcripts, optionals = [], [], []
    for _s in range(S):
        while True:
            L = int(rng.integers(1, max_L + 1))
            units = rng.integers(0, len(RANDOM_NS), L).astype(np.int32)
            if max_slots is None or slots_of([RANDOM_NS[k] for k in units]) <= max_slots:
                break
        opt = np.zeros(L, np.uint8)
        for l in range(L):
            opt[l] = rng.uniform() < 0.3 and not (l > 0 and opt[l - 1])
        if opt.all():
            opt[int(rng.integers(0, L))] = 0
        T = int(rng.integers(max(1, L - 2), L + 150 + 1))
        streams.append(rng.integers(0, M, T).astype(np.uint16))
        transcripts.append(units)
        optionals.append(opt)
    return models, streams, transcripts, optionals


def small_models(seed=3, Ns=(5, 3, 4), zeros=0.3):
    rng = np.random.default_rng(seed)
    return [random_model(rng, N, M, zeros) for N in Ns]


def uniform_model(N, m=M):
    return np.full(N, 1.0 / N), np.full((N, N), 1.0 / N), np.full((N, m), 1.0 / m)


def skip_tie_models():
    """a uniform model, and one that cannot emit symbol 1"""
    pi, A, B = uniform_model(2, 4)
    picky = B.copy()
    picky[:, 1] = 0.0
    return [(pi, A, B), (pi, A, picky)]


def skip_tie():
    """-> (stream, units, optional) under skip_tie_models(): passing over the optional unit 1 ties with using it"""
    return np.array([0, 1, 2], np.uint16), np.array([0, 0, 1], np.int32), np.array([0, 1, 0], np.uint8)


# ---- the planted stream ------------------------------------------------------------------------------------------------------
PLANTED_ORDER = [0, 2, 1, 0, 0, 1, 2]  # (the same class twice in a row included)
FILLER = 3
PEAKS = [[0, 1, 2], [3, 4, 5], [1, 3, 5]]  # the symbol each state leans to: no unit ends on the symbol the next one starts with


def planted_models():
    """three left-to-right models of 3 states whose states lean to symbols of their own, and a one-state filler"""
    models = []
    for k in range(3):
        pi = np.array([1.0, 0.0, 0.0])
        A = np.array([[0.8, 0.2, 0.0], [0.0, 0.8, 0.2], [0.0, 0.0, 1.0]])
        B = np.full((3, M), 0.02)
        for j in range(3):
            B[j, PEAKS[k][j]] = 0.86
        models.append((pi, A, B / B.sum(axis=1, keepdims=True)))
    Bf = np.full((1, M), 0.04)
    Bf[0, 6:] = 0.38
    models.append((np.ones(1), np.ones((1, 1)), Bf / Bf.sum()))
    return models


def planted(fill, seed=20):
    """fill: "all" (a filler run before, between and after all units), "none", or "some" (each with probability 1/2)
    -> (stream, units, optional, truth) -- the transcript has the optional filler everywhere; truth[l] = (begin, end) of
    unit l of that transcript, (-1, -1) for a filler that was not sampled"""
    rng = np.random.default_rng(seed)
    models = planted_models()
    sym, units, optional, truth = [], [], [], []

    def emit(k, durations):
        b = len(sym)
        for j, n in enumerate(durations):
            sym.extend(rng.choice(M, size=n, p=models[k][2][j]).tolist())
        return b, len(sym)

    def filler():
        units.append(FILLER)
        optional.append(1)
        present = fill == "all" or (fill == "some" and rng.uniform() < 0.5)
        truth.append(emit(FILLER, [int(rng.integers(6, 14))]) if present else (-1, -1))

    filler()
    for k in PLANTED_ORDER:
        units.append(k)
        optional.append(0)
        truth.append(emit(k, rng.integers(4, 10, 3).tolist()))
        filler()
    return (np.array(sym, dtype=np.uint16), np.array(units, dtype=np.int32), np.array(optional, dtype=np.uint8),
            np.array(truth, dtype=np.int64))
