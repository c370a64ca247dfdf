"""inputs that test_hmm_embedded_cpu.py and test_gpu_hmm_embedded.py share (TEST INFRASTRUCTURE): the packings, models and
planted streams of tests/hmm_align_cases.py, the blurred start of the EM tests, and the batch the GPU tests run twice."""
import numpy as np

from . import hmm_align_cases as A

M = A.M
PACKINGS = A.PACKINGS
packing = A.packing
small_models = A.small_models
planted = A.planted
planted_models = A.planted_models
PEAKS = A.PEAKS
PLANTED_ORDER = A.PLANTED_ORDER
FILLER = A.FILLER
SHAPES = A.SHAPES
shape = A.shape
slots_of = A.slots_of
embed_route = A.embed_route
event_models = A.event_models
event_batch = A.event_batch
unlike_streams = A.unlike_streams
random_batch = A.random_batch


def pack(streams, transcripts, optionals=None):
    """-> sym, offs, units, unit_offs, optional as the entry points take them"""
    sym = np.concatenate([np.asarray(s, dtype=np.uint16) for s in streams]) if streams else np.zeros(0, np.uint16)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    units = np.concatenate([np.asarray(u, dtype=np.int32) for u in transcripts]).astype(np.int32)
    unit_offs = np.concatenate([[0], np.cumsum([len(u) for u in transcripts])]).astype(np.int64)
    opt = None if optionals is None else np.concatenate([np.asarray(o, dtype=np.uint8) for o in optionals]).astype(np.uint8)
    return sym, offs, units, unit_offs, opt


def blurred(models, w=0.5):
    """every model mixed (1 - w) : w with the uniform model of its own type: B with the uniform row, pi and the rows of A with
    the uniform distribution over their own support, so that the zeros of a left-to-right model stay zeros"""
    out = []
    for pi, Am, B in models:
        pi, Am, B = (np.asarray(x, dtype=np.float64) for x in (pi, Am, B))
        sup = lambda x: (x > 0) / np.maximum((x > 0).sum(axis=-1, keepdims=True), 1)
        out.append(((1 - w) * pi + w * sup(pi), (1 - w) * Am + w * sup(Am), (1 - w) * B + w / B.shape[1]))
    return out


def planted_batch(fills=("some", "all"), seeds=(20, 21, 22)):
    """streams sampled from the planted models, every transcript with the optional filler everywhere
    -> (streams, transcripts, optionals)"""
    streams, transcripts, optionals = [], [], []
    for fill in fills:
        for seed in seeds:
            s, u, o, _truth = planted(fill, seed)
            streams.append(s)
            transcripts.append(u)
            optionals.append(o)
    return streams, transcripts, optionals
