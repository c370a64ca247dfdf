"""inputs that test_hmm_align_posteriors_looped_cpu.py and test_gpu_hmm_align_posteriors_looped.py share (TEST INFRASTRUCTURE):
the cases of the looped body of `hmm align --posteriors` (ECOZ2_HMM_ALIGN_POSTERIOR_BODY), and the LDS
arithmetic of hmm_align_posterior_looped.hip, restated."""
from . import hmm_align_cases as cases
from .hmm_embedded_looped_cases import (RANDOM_MAX_L, RANDOM_SEED, SEG_LDS_BYTES, SEG_MAX_WAVES, embed_looped_lds_bytes,  # noqa: F401
                                        thirty_three_slots, too_large)

BODY = "ECOZ2_HMM_ALIGN_POSTERIOR_BODY"
UNIT_SUM_BYTES = 3 * 8  # w0, w1, w2 of a unit


def align_post_looped_lds_bytes(max_L, max_slots, max_sumN, a_words, a_lds):
    """the looped E-step's mandatory part (2 x max_slots partial sums, V / R of two steps, two per-state arrays) and A, and the
    three per-unit sums"""
    return embed_looped_lds_bytes(max_L, max_slots, max_sumN, a_words, a_lds, False) + UNIT_SUM_BYTES * max_L


def looped_route(Ns, L, slots, sumN):
    """-> a_lds as post_plan decides it for a looped launch of one stream when it is not forced"""
    a_words = sum(N * (N | 1) for N in Ns)
    return align_post_looped_lds_bytes(L, slots, sumN, a_words, True) <= SEG_LDS_BYTES


def case(name):
    """-> (models, units, optional or None, stream) of a packing, a shape or the 33-slot case"""
    if name == "33 slots":
        models, units, stream = thirty_three_slots()
        return models, units, None, stream
    if name in cases.PACKINGS:
        models, units, stream = cases.packing(name)
        return models, units, None, stream
    return cases.shape(name)
