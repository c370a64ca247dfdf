"""Inputs for the launch shapes of the batched HMM trainer (train_grid_batch) that small corpora never
reach, and the host's launch rules restated in Python, so that a test can prove from its inputs that a case reaches the
shape it names.  Used by test_hmm_learn_grid_cases_cpu.py (oracle only) and test_gpu_hmm_learn_grid_shapes.py.

A case is a dict: models [(pi, A, B)], seqs [uint16 arrays], ranges [(lo, hi)], eps, val_auto, maxit, and per case
what its tests need (`bad`: {model index: {index within the model's range: kind}}).  Every case is seeded: the oracle's
generator for the initial models, numpy's for the sequences.

Symbols >= M.  e2vq_hmm_train_grid refuses a symbol >= M_k in model k's range before the device;
e2vq_hmm_train_classes and e2vq_hmm_train do not look.  A case with 'range' sequences therefore carries `seqs` as
built, for the entry points that admit them, and `grid_seqs`, in which each such symbol is replaced by the case's
unemittable symbol: the same slots hold bad sequences, of kind 'emit' instead."""
import numpy as np

from tests.test_gpu_hmm_shapes import _bad_mix
from tests.test_hmm_counts_cpu import _without_column

# ---- the host rules (hmm_device.hip, hmm_train.cpp, hmm_model.cpp) ------------------------------------------------
WAVE_N = 64        # N <= 64: k_hmm_fb_grid, one wave per sequence; above: launch_fb (k_hmm_fb_wg), one workgroup per sequence
FB_WAVES = 4       # waves of a k_hmm_fb_grid workgroup
FB_MAX_WG = 2048   # workgroups of one model at the most
FB_WG_GRID = 64    # workgroups of k_hmm_fb_wg
GRID_Y = 65535     # models of one M-step launch


def fb_class_workgroups(S):
    """workgroups of a model of N <= 64 with S sequences"""
    return min(max(-(-S // FB_WAVES), 1), FB_MAX_WG)


def wave_slot(i, S):
    """N <= 64: sequence i of a model's S -> (workgroup, wave in it, turn): `for (s = s_lo + wg*4 + wib; s < s_hi; s += nwg*4)`"""
    W = fb_class_workgroups(S) * FB_WAVES
    return (i % W) // FB_WAVES, (i % W) % FB_WAVES, i // W


def wave_turns(S):
    """N <= 64: how many sequences each wave of the model takes, {(workgroup, wave): turns}, idle waves included"""
    nwg = fb_class_workgroups(S)
    W = nwg * FB_WAVES
    return {(g // FB_WAVES, g % FB_WAVES): len(range(g, S, W)) for g in range(W)}


def wg_slot(i, S):
    """N > 64: sequence i of a model's S -> (workgroup, turn)"""
    G = min(S, FB_WG_GRID)
    return i % G, i // G


def blocks_table(Ns, Ss, active):
    """the (model, workgroup, workgroup count) table of one iteration and its launches: -> (rows, [(N, at, count)]);
    models of N <= 64 only, grouped by N ascending, in model order within an N"""
    rows, launches = [], []
    for N in sorted({Ns[k] for k in active if Ns[k] <= WAVE_N}):
        at = len(rows)
        for k in active:
            if Ns[k] == N:
                nb = fb_class_workgroups(Ss[k])
                rows += [(k, b, nb) for b in range(nb)]
        launches.append((N, at, len(rows) - at))
    return rows, launches


def merged_runs(ranges):
    """BatchSeqs: the ranges sorted and merged where they overlap or touch -> ([(lo, hi)], [first batch index of each])"""
    runs = []
    for lo, hi in sorted(ranges):
        if runs and lo <= runs[-1][1]:
            runs[-1][1] = max(runs[-1][1], hi)
        else:
            runs.append([lo, hi])
    at, n = [], 0
    for lo, hi in runs:
        at.append(n)
        n += hi - lo
    return [tuple(r) for r in runs], at


def local_index(ranges, s):
    """BatchSeqs::local: the batch index of store sequence s"""
    runs, at = merged_runs(ranges)
    q = max(i for i, (lo, _hi) in enumerate(runs) if lo <= s)
    return at[q] + (s - runs[q][0])


def grid_y_launches(n_active):
    """launch_reestimate_grid: models per launch"""
    return [min(GRID_Y, n_active - k0) for k0 in range(0, n_active, GRID_Y)]


def grid_admissible(seqs, M, k_bad):
    """every symbol >= M replaced by k_bad (see the module's text)"""
    return [np.where(s >= M, k_bad, s).astype(np.uint16) for s in seqs]


def slice_of(case, k, key="seqs"):
    lo, hi = case["ranges"][k]
    return case[key][lo:hi]


def _class(rng, M, lens, k_bad, bad_at, same_wave):
    """_bad_mix with the sequences that share a wave (or workgroup) with a bad one kept good: at least one symbol"""
    lens = np.array(lens)
    for i in bad_at:
        for j in same_wave(i):
            if j not in bad_at:
                lens[j] = max(lens[j], 1)
    return _bad_mix(rng, M, lens, k_bad, bad_at)


# ---- 1. persistent_mid -----------------------------------------------------------------------------------------------
S_B, S_D = 2 * 8192 + 37, 8192 + 300
BAD_B = {3: "empty", 4: "range", 5: "emit",                               # first turn of waves that take three
         8192 + 10: "empty", 8192 + 11: "range", 8192 + 12: "emit",       # second turn, good before and after
         2 * 8192 + 20: "empty", 2 * 8192 + 21: "range", 2 * 8192 + 22: "emit",  # third turn
         50: "emit", 8192 + 60: "range"}                                  # waves that take two: bad-good, good-bad
BAD_D = {5: "empty", 6: "range", 7: "emit", 8192 + 100: "empty", 8192 + 101: "range", 8192 + 102: "emit"}


def persistent_mid(H):
    H.seed(4101)
    rng = np.random.default_rng(4101)
    M, k_bad = 8, 7
    a = _bad_mix(rng, M, rng.integers(2, 9, 7), k_bad, {})
    b = _class(rng, M, rng.integers(0, 7, S_B), k_bad, BAD_B, lambda i: range(i % 8192, S_B, 8192))
    c = [rng.integers(0, 12, n).astype(np.uint16) for n in rng.integers(2, 9, 13)]
    d = _class(rng, M, rng.integers(0, 4, S_D), k_bad, BAD_D, lambda i: range(i % 8192, S_D, 8192))
    seqs, ranges_of = [], {}
    for name, cls in (("a", a), ("b", b), ("c", c), ("d", d)):
        ranges_of[name] = (len(seqs), len(seqs) + len(cls))
        seqs += cls
    spec = [(5, 8, 3, "a"), (5, 8, 0, "b"), (5, 12, 3, "c"), (3, 8, 3, "b"), (64, 8, 3, "d")]
    models = []
    for N, Mk, typ, name in spec:
        pi, A, B = H.init(N, Mk, typ)
        models.append((pi, A, _without_column(B, k_bad) if name in "bd" else B))
    return dict(models=models, seqs=seqs, grid_seqs=grid_admissible(seqs, M, k_bad), ranges=[ranges_of[s[3]] for s in spec],
                eps=1e-5, val_auto=0.3, maxit=2, bad={1: BAD_B, 3: BAD_B, 4: BAD_D}, k_bad=k_bad,
                classes_groups=[[0, 1], [4]])  # (the models that share N and M, and the N = 64 one alone)


# ---- 2. blocks_mix ---------------------------------------------------------------------------------------------------
MIX_NS, MIX_SIZES = (2, 21, 64), (1, 4, 5, 33, 8193)
MIX_VAL_AUTO = 100.0  # (L is a sum over up to 8193 sequences: between the second gains of the big class at N = 21 and at N = 2)


def blocks_mix(H):
    """class-major model order, so the models of one N are never neighbours in the call.  The one-sequence class is one
    drifting sequence of 4000 symbols (large gains for several iterations), the 4-sequence class four copies of a
    constant one (converged after the first M-step), the 8193-sequence class random ones of 1 to 3 symbols."""
    H.seed(4202)
    rng = np.random.default_rng(4202)
    M = 8
    classes = [[np.clip((np.linspace(0, M - 1, 4000) + rng.normal(0, 1.5, 4000)).round(), 0, M - 1).astype(np.uint16)],
               [np.full(3, 2, np.uint16) for _ in range(4)],
               [rng.integers(0, M, n).astype(np.uint16) for n in rng.integers(4, 12, 5)],
               [rng.integers(0, M, n).astype(np.uint16) for n in rng.integers(1, 9, 33)],
               [rng.integers(0, M, n).astype(np.uint16) for n in rng.integers(1, 4, 8193)]]
    assert tuple(len(c) for c in classes) == MIX_SIZES
    seqs, cls_range = [], []
    for cls in classes:
        cls_range.append((len(seqs), len(seqs) + len(cls)))
        seqs += cls
    models, ranges = [], []
    for r in cls_range:
        for N in MIX_NS:
            models.append(H.init(N, M, 3))
            ranges.append(r)
    return dict(models=models, seqs=seqs, ranges=ranges, eps=1e-5, val_auto=MIX_VAL_AUTO, maxit=4)


# ---- 3. ranges -------------------------------------------------------------------------------------------------------
RANGES = [(60, 100), (0, 10), (30, 31), (65, 90), (60, 100)]
RANGES_NM = [(4, 12), (3, 6), (2, 9), (4, 14), (6, 12)]
POISON, POISON_SYMBOL = 45, 60000


def ranges_case(H):
    """sequences 10..29 and 31..59 belong to nobody: ordinary ones, each different from every used one, and POISON,
    which holds a symbol above every M"""
    H.seed(4303)
    rng = np.random.default_rng(4303)
    top = lambda s: 9 if s == 30 else (12 if s >= 60 else 6)  # (nobody's: symbols every model takes)
    seqs = [rng.integers(0, top(s), int(rng.integers(8, 16))).astype(np.uint16) for s in range(100)]
    seqs[POISON] = np.array([1, POISON_SYMBOL, 2], np.uint16)
    return dict(models=[H.init(N, M, 3) for N, M in RANGES_NM], seqs=seqs, ranges=list(RANGES), eps=1e-5, val_auto=0.3, maxit=3)


# ---- 4. big_n_scratch ------------------------------------------------------------------------------------------------
BIG_NS, BIG_S = (65, 141, 142, 200), 70
BAD_BIG = {FB_WG_GRID + 1: "empty", FB_WG_GRID + 2: "range", FB_WG_GRID + 3: "emit"}  # the second turn of workgroups 1, 2, 3


def big_n_scratch(H):
    H.seed(4404)
    rng = np.random.default_rng(4404)
    M, k_bad = 8, 7
    seqs = [rng.integers(0, M, 4).astype(np.uint16) for _ in range(3)]  # (nobody's: no range starts at 0)
    models, ranges = [], []
    for N, typ in zip(BIG_NS, (0, 3, 3, 2)):
        cls = _class(rng, M, rng.integers(0, 10, BIG_S), k_bad, BAD_BIG, lambda i: range(i % FB_WG_GRID, BIG_S, FB_WG_GRID))
        ranges.append((len(seqs), len(seqs) + BIG_S))
        seqs += cls
        pi, A, B = H.init(N, M, typ)
        models.append((pi, A, _without_column(B, k_bad)))
    return dict(models=models, seqs=seqs, grid_seqs=grid_admissible(seqs, M, k_bad), ranges=ranges, eps=1e-5, val_auto=0.3,
                maxit=2, bad={k: BAD_BIG for k in range(4)}, k_bad=k_bad, classes_groups=[[0], [1], [2], [3]])


# ---- 5. many_models --------------------------------------------------------------------------------------------------
MANY_K, MANY_CLASSES, MANY_VARIANTS = GRID_Y + 3, 4, 5


def many_models(H):
    """-> the case with its 20 distinct (class, variant) pairs only (`pairs`: [(pi, A, B, range)], pair_of(k) -> index);
    the K models of the call are models_of(case)"""
    H.seed(4505)
    rng = np.random.default_rng(4505)
    M = 4
    seqs, cls_range = [], []
    for c in range(MANY_CLASSES):
        cls = [rng.integers(0, M, int(rng.integers(2, 6))).astype(np.uint16) for _ in range(2 + c % 2)]
        cls_range.append((len(seqs), len(seqs) + len(cls)))
        seqs += cls
    variants = [H.init(1, M, 3) for _ in range(MANY_VARIANTS)]
    pairs = [(variants[v], cls_range[c]) for c in range(MANY_CLASSES) for v in range(MANY_VARIANTS)]
    return dict(pairs=pairs, seqs=seqs, eps=1e-5, val_auto=0.3, maxit=2)


def many_pair_of(k):
    return (k % MANY_CLASSES) * MANY_VARIANTS + k % MANY_VARIANTS


def many_models_of(case):
    """(models, ranges) of the K-model call: model k trains on class k mod 4 from variant k mod 5"""
    idx = [many_pair_of(k) for k in range(MANY_K)]
    return [case["pairs"][i][0] for i in idx], [case["pairs"][i][1] for i in idx]


# ---- the oracle on a case --------------------------------------------------------------------------------------------
def oracle_train(H, case, k, key="seqs", seqs=None):
    """H.learn of model k on its slice -> (pi, A, B, hist)"""
    return H.learn(*case["models"][k], slice_of(case, k, key) if seqs is None else seqs, case["eps"], case["val_auto"], case["maxit"])


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """two (pi, A, B, hist) results equal on their 64 bits"""
    return (len(a[3]) == len(b[3]) and np.array_equal(bits(a[3]), bits(b[3]))
            and all(x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a[:3], b[:3])))


BUILDERS = dict(persistent_mid=persistent_mid, blocks_mix=blocks_mix, ranges=ranges_case, big_n_scratch=big_n_scratch)
_REFERENCE = {}


def reference(H, name):
    """the case with the oracle's results, computed once per process and shared (leave them unchanged): case["want"][k]
    is model k trained on its slice of what the grid call gets (`grid_seqs` where the case has them); case["want_as_built"]
    holds, for the models of `classes_groups`, the result on `seqs` as built ('range' sequences included).  Empty
    sequences stay in the slices: e2h_learn takes T = 0 (status 1, counted as skipped, nothing added)."""
    if name not in _REFERENCE:
        case = BUILDERS[name](H)
        key = "grid_seqs" if "grid_seqs" in case else "seqs"
        case["want"] = [oracle_train(H, case, k, key) for k in range(len(case["models"]))]
        case["want_as_built"] = {k: oracle_train(H, case, k) for g in case.get("classes_groups", []) for k in g}
        _REFERENCE[name] = case
    return _REFERENCE[name]


def many_reference(H):
    """many_models with the oracle's result of each of its 20 pairs (case["want"][pair])"""
    if "many_models" not in _REFERENCE:
        case = many_models(H)
        case["want"] = [H.learn(*m, case["seqs"][lo:hi], case["eps"], case["val_auto"], case["maxit"]) for m, (lo, hi) in case["pairs"]]
        _REFERENCE["many_models"] = case
    return _REFERENCE["many_models"]
