"""inputs that test_hmm_embedded_looped_cpu.py and test_gpu_hmm_embedded_looped.py share (TEST INFRASTRUCTURE): the cases of
the looped body of the embedded E-step (ECOZ2_HMM_EMBED_BODY), and the LDS arithmetic of
hmm_embed_looped.hip, restated."""
import numpy as np

from . import hmm_embedded_cases as cases

BODY = "ECOZ2_HMM_EMBED_BODY"
SEG_LDS_BYTES = 160 * 1024
SEG_MAX_WAVES = 16
RANDOM_SEED, RANDOM_MAX_L = 24, 40  # the batch test_gpu_hmm_align_shapes.py documents


def embed_looped_lds_bytes(max_L, max_slots, max_sumN, a_words, a_lds, an_lds):
    """2 x max_slots partial sums, V / R of two steps, two per-state arrays; then A and the AN limb table"""
    return (2 * max_slots * 8 + 2 * max_L * 8 + 2 * max_sumN * 8 + (a_words * 8 if a_lds else 0) + (a_words * 16 if an_lds else 0))


def looped_route(Ns, L, slots, sumN):
    """-> (a_lds, an_lds) as embed_plan decides them for a looped launch of one stream with neither forced"""
    a_words = sum(N * (N | 1) for N in Ns)
    a_lds = embed_looped_lds_bytes(L, slots, sumN, a_words, True, False) <= SEG_LDS_BYTES
    return a_lds, embed_looped_lds_bytes(L, slots, sumN, a_words, a_lds, True) <= SEG_LDS_BYTES


def thirty_three_slots():
    """-> (models, units, stream): 33 units cycling over three 64-state classes, T = 100: a wave takes three slots"""
    models = cases.packing("64x17")[0]
    units = np.array([l % 3 for l in range(33)], dtype=np.int32)
    rng = np.random.default_rng(33)
    runs = rng.integers(0, cases.M, 26)
    stream = np.where(rng.uniform(size=100) < 0.7, np.repeat(runs, 4)[:100], rng.integers(0, cases.M, 100)).astype(np.uint16)
    return models, units, stream


def too_large():
    """-> (N, L, slots, sumN) of a transcript whose mandatory part does not fit: 3 000 units of one 3-state class"""
    N, L = 3, 3000
    slots = cases.slots_of([N] * L)
    assert embed_looped_lds_bytes(L, slots, N * L, 0, False, False) > SEG_LDS_BYTES
    return N, L, slots, N * L
