"""what test_hmm_posteriors_looped_cpu.py and test_gpu_hmm_posteriors_looped.py share (TEST INFRASTRUCTURE): the looped body
of `hmm segment --posteriors` (ECOZ2_HMM_POSTERIOR_BODY, hmm_posterior_looped.hip) -- the restatement without
its cap of 16 wave-slots, the class sets above 16 slots, the copies of the resident sets, and the LDS formula restated."""
import contextlib
import functools

import numpy as np

from . import hmm_class_loop_cases as loop_cases
from . import hmm_posterior_restatement as R

NINF = float("-inf")
BODY = "ECOZ2_HMM_POSTERIOR_BODY"
CHUNK = "ECOZ2_HMM_POSTERIOR_CHUNK_BYTES"
SEG_LDS_BYTES = loop_cases.SEG_LDS_BYTES
SEG_MAX_WAVES = loop_cases.SEG_MAX_WAVES
LENGTHS = (0, 1, 2, 63, 64, 65, 129)
SWITCHES = (NINF, -3.0, 0.0)


# ---- the restatement at any number of slots ------------------------------------------------------------------------------------
@contextlib.contextmanager
def _uncapped():
    """posteriors_one asserts slots <= MAX_SLOTS, the resident body's limit; GS itself is defined for any number of slots"""
    before = R.MAX_SLOTS
    R.MAX_SLOTS = 1 << 30
    try:
        yield
    finally:
        R.MAX_SLOTS = before


def posteriors_one(models, seq, ln_switch):
    with _uncapped():
        return R.posteriors_one(models, seq, ln_switch)


def posteriors(models, sym, offs, ln_switch):
    """hmm_posterior_restatement.posteriors without the cap: the layout of ecoz2rs_amd.hmm.segment_posteriors"""
    with _uncapped():
        return R.posteriors(models, sym, offs, ln_switch)


# ---- class sets above 16 slots -------------------------------------------------------------------------------------------------
# name: (N of every class, M).  waves = min(slots, 16); a wave serves ceil or floor of slots / 16 slots.
WIDE = {
    "33x17": ((33,) * 17, 8),       # 17 slots of one class each (v_readlane chains); wave 0 serves two; A (145 KB) still in LDS
    "5x193": ((5,) * 193, 300),     # 17 slots, twelve classes to a slot (ds_bpermute chains), the last slot holds one class of 5
    "33x33": ((33,) * 33, 8),       # 33 slots: wave 0 serves three, the others two; A (281 KB) stays in global memory
    "64x20": ((64,) * 20, 300),     # the headline shape: 20 full slots, A (650 KB) in global memory
    # 18 slots -- (64), (20, 20, 20), (33) six times, the last 33 shares its slot with three of 7: one-class slots next to
    # packed ones, waves 0 and 1 serve two slots and the other fourteen one
    "mixed": ((64, 20, 20, 20, 33) * 6 + (7, 7, 7), 8),
}
# the class sets of test_gpu_hmm_posteriors.py, where the resident body runs
RESIDENT = {
    "1": [1], "5": [5], "1_1": [1, 1], "5x3": [5] * 3, "5x12": [5] * 12, "5x13": [5] * 13, "21_22_64": [21, 22, 64],
    "21x3": [21] * 3, "64x16": [64] * 16,
}


def slots_of(Ns):
    return int(R.packing(Ns)[2])


def a_words(Ns):
    return sum(N * (N | 1) for N in Ns)


def wide_models(name):
    """leaning models with exact zeros in pi, A and B: terms of mixed magnitude in every sum"""
    Ns, M = WIDE[name]
    return loop_cases.leaning_models(17 + len(Ns), Ns, M)


def streams(seed, M, lengths=LENGTHS, K=None):
    """a stream per length: run streams (the symbols K classes lean to) in turn with uniform symbols"""
    rng = np.random.default_rng(seed)
    out = []
    for i, T in enumerate(lengths):
        if K is not None and i % 2:
            out.append(loop_cases.run_stream(seed + i, K, M, T))
        else:
            out.append(rng.integers(0, M, T).astype(np.uint16))
    return out


def pack(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    sym = np.concatenate(seqs).astype(np.uint16) if seqs else np.zeros(0, np.uint16)
    return sym, offs


@functools.lru_cache(maxsize=None)
def wide_case(name):
    """-> (models, sym, offs) of a row of WIDE (read only: the tests share it)"""
    Ns, M = WIDE[name]
    sym, offs = pack(streams(len(Ns), M, K=len(Ns)))
    return wide_models(name), sym, offs


@functools.lru_cache(maxsize=None)
def wide_reference(name, ln_switch):
    models, sym, offs = wide_case(name)
    return posteriors(models, sym, offs, ln_switch)


# ---- the LDS of the looped body, restated; test_hmm_posteriors_looped_cpu.py holds it against the source ------------------------
def posteriors_looped_lds_bytes(slots, sumN, a_words_, a_lds):
    """mandatory: the partial sums of GS in both parities and one double per composite state; A behind them where it fits"""
    return 2 * slots * 8 + sumN * 8 + (a_words_ * 8 if a_lds else 0)


def looped_route(Ns):
    """-> dict waves, a_lds, lds, c_copies: what launch_loop_posteriors_looped decides for the class set"""
    slots, sumN, aw = slots_of(Ns), sum(Ns), a_words(Ns)
    a_lds = posteriors_looped_lds_bytes(slots, sumN, aw, True) <= SEG_LDS_BYTES
    waves = min(slots, SEG_MAX_WAVES)
    return dict(waves=waves, a_lds=a_lds, lds=posteriors_looped_lds_bytes(slots, sumN, aw, a_lds), c_copies=waves)


def most_mandatory_lds():
    """the largest mandatory LDS a class set that segment_check_shape admits (N <= 64, sum N <= 4096) can ask for: two
    neighbouring slots hold more than 64 states between them (else the second's first class had fitted the first), so
    slots <= 2 * 4096 / 64 + 1"""
    sumN = loop_cases.SEG_MAX_SUM_N
    return posteriors_looped_lds_bytes(2 * sumN // 64 + 1, sumN, 0, False)
