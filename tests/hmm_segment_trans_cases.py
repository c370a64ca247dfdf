"""inputs that test_hmm_segment_trans_cpu.py and test_gpu_hmm_segment_trans.py share (TEST INFRASTRUCTURE): the models,
streams and price matrices of the uniform-matrix equivalence of DESIGN.md 4.8.8.  The CPU test asserts for every case that
the two restatements agree in the path as well; the GPU test then compares the two decoders' paths on the same inputs."""
import numpy as np

NINF = float("-inf")
UNIFORM_PRICE = -5.0


def random_rows(rng, n, m, zeros=0.0):
    """n distributions over m outcomes; `zeros`: the share of entries set to 0 (a row keeps at least one entry)"""
    x = rng.uniform(0.05, 1.0, (n, m))
    if zeros:
        x[rng.uniform(size=(n, m)) < zeros] = 0.0
        x[np.arange(n), rng.integers(0, m, n)] += 0.5
    return x / x.sum(axis=1, keepdims=True)


def random_model(rng, N, M, zeros=0.0):
    return random_rows(rng, 1, N, zeros)[0], random_rows(rng, N, N, zeros), random_rows(rng, N, M)


def random_prices(rng, K, forbidden=0.2):
    """an asymmetric K x K matrix of prices in (-6, 0], a share of them -inf"""
    lt = -rng.uniform(0.0, 6.0, (K, K))
    lt[rng.uniform(size=(K, K)) < forbidden] = NINF
    return lt


def uniform_cases():
    """[(name, models, streams)]: dense and sparse models, duplicated classes (exact ties), one and several classes a wave"""
    out = []
    for name, Ns, zeros, dup, seed in (("dense", (3, 5, 4), 0.0, False, 1), ("sparse", (4, 4, 2, 6), 0.5, False, 2),
                                       ("duplicated", (5, 3, 5, 3), 0.0, True, 3), ("wide", (40, 40, 7), 0.3, False, 4)):
        rng = np.random.default_rng(seed)
        M = 8
        models = [random_model(rng, N, M, zeros) for N in Ns]
        if dup:
            models[2], models[3] = models[0], models[1]
        streams = [rng.integers(0, M, n).astype(np.uint16) for n in (1, 2, 65, 119)]
        out.append((name, models, streams))
    return out
