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
