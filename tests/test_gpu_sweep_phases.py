"""The stage-1 token of the fused sorted pass changes WHEN a wave enters its stage 1, never what it computes.

Whole ladders through the two instantiations that carry the token -- two blocks per turn (ECOZ2_VQ_ACCUMULATE=sorted) and one
(the default path on a shard of fewer than 4 096 blocks) -- on frame counts that leave the last block and the last turn
partial (20 000, 20 000 + 37: one wave of a SIMD pair runs out of turns before the other) or give most waves no turn at all
(130 frames: three blocks), on the 20-class generator and on the continuum without classes (which flags every tile), at
P = 36 and at a smaller order.  Per case the codebook's bytes, every level's pass count and DD, and the symbols of one more pass
must equal those of the same ladder on the plain FP64 sweep (`set_prefilter(False)`) -- and those of the same prefiltered
ladder run a second time: a result that depended on the waves' timing would not repeat."""
import ctypes as C

import numpy as np
import pytest

import ecoz2rs_amd as e

pytestmark = pytest.mark.gpu

T_MAX = 20000 + 37
_frames_of = {}
_plain_of = {}


def _frames(gen, Pn, T):
    """the first T frames of the stream (generated once per generator and order)"""
    if (gen, Pn) not in _frames_of:
        _frames_of[gen, Pn] = (e.synth.synth_frames(20401, 20, Pn, 0, T_MAX) if gen == "classes"
                               else e.synth.synth_frames_kind(20402, 1, 6, 0.01, Pn, 0, T_MAX))
    return _frames_of[gen, Pn][:T]


def _symbols_of_one_more_pass(s, T):
    ptr = C.c_void_p()
    assert e.lib.hipSetDevice(0) == 0
    assert e.lib.hipMalloc(C.byref(ptr), C.c_size_t(2 * T)) == 0
    try:
        assert e.lib.hipMemset(ptr, 0xFF, C.c_size_t(2 * T)) == 0
        s.run_pass(ptr.value, None)
        s.synchronize()
        out = np.empty(T, dtype=np.uint16)
        assert e.lib.hipMemcpy(out.ctypes.data_as(C.c_void_p), ptr, C.c_size_t(2 * T), 2) == 0  # D2H
    finally:
        e.lib.hipFree(ptr)
    return out.tobytes()


def _ladder(frames, Pn, max_m, prefilter):
    """(codebook bytes, ((M, passes, DD.hex()) per level), symbols of one more pass), and the sweeps the level passes ran"""
    kinds = []
    with e.VqSession(Pn) as s:
        s.set_frames(frames)
        s.prepare()
        s.init_codebook()
        if not prefilter:
            s.set_prefilter(False)
        levels = s.learn(0.05, max_m, callback=lambda *_a: kinds.append(s.last_pass_sweep()[:2]))
        cb = s.get_codebook().tobytes()
        sym = _symbols_of_one_more_pass(s, frames.shape[0])
    return (cb, tuple((l.M, l.passes, l.DD.hex()) for l in levels), sym), kinds


def _plain(gen, Pn, T, max_m, monkeypatch):
    """the reference of a case: the plain FP64 sweep (computed once, shared by the launch shapes, left unchanged)"""
    key = (gen, Pn, T, max_m)
    if key not in _plain_of:
        monkeypatch.delenv("ECOZ2_VQ_ACCUMULATE", raising=False)
        _plain_of[key] = _ladder(_frames(gen, Pn, T), Pn, max_m, prefilter=False)[0]
    return _plain_of[key]


CASES = [(36, gen, T, max_m, acc) for gen in ("classes", "continuum") for T in (20000, T_MAX, 130) for max_m in (256, 1024)
         for acc in ("sorted", "default")]
# a smaller order (rows of 21 coefficients: the waves' regions leave room for two workgroups on a CU)
CASES += [(20, gen, T, 1024, acc) for gen in ("classes", "continuum") for T in (T_MAX, 130) for acc in ("sorted", "default")]


@pytest.mark.parametrize("Pn,gen,T,max_m,acc", CASES)
def test_ladder_equals_the_plain_sweep_and_repeats(monkeypatch, Pn, gen, T, max_m, acc):
    monkeypatch.setenv("ECOZ2_VQ_QUIET", "1")
    frames = _frames(gen, Pn, T)
    want = _plain(gen, Pn, T, max_m, monkeypatch)
    if acc == "sorted":
        monkeypatch.setenv("ECOZ2_VQ_ACCUMULATE", "sorted")  # (the fused sorted pass from M = 64 on, two blocks per turn)
    else:
        monkeypatch.delenv("ECOZ2_VQ_ACCUMULATE", raising=False)  # (from M = 256 on, one block per turn: 313 blocks or 3)
    first, kinds = _ladder(frames, Pn, max_m, prefilter=True)
    again, _kinds = _ladder(frames, Pn, max_m, prefilter=True)
    for name, a, b, c in zip(("codebook", "passes and DD", "symbols"), first, again, want):
        assert a == c, f"{name}: differs from the plain sweep"
        assert a == b, f"{name}: the second run of the same ladder differs"
    if gen == "classes" and T >= 20000:
        # the kernel under test did run: fused pass over grouped frames (kind 3), two stages
        assert (3, True) in kinds, kinds
