"""Shared inputs and the CPU reference of the `vq classify` tests (test_vq_classify_cases_cpu.py, test_gpu_vq_classify.py).

Nothing here needs a device: the frames come from the library's host-side generator, the distortions from the CPU oracle
(tests/oracle_lib.py), and the unit plan and the report are restated from ecoz2_vq_classify (vq_entry.cpp).

Scores: for file k and codebook i, a Python-float loop over the oracle's dmin in frame order, `e += d - 1.0`, then `e / T`
-- the sum ecoz2_vq_classify keeps across its units, written from the oracle's output, never from the library's.

Sensitivity: '%g' shows six digits, so every file of two or more frames carries PLANTED frames at the places where the host
code could lose, double or misplace a frame: its first and last frame (which are also the first and last frame of its batched
segment) and the frame on each side of every cut at the chunk sizes the tests run (1024 and 1500).  A planted frame is a
frame of another generator seed, scaled by a power of two so that its dmin - 1 is at least 100 times the file's median under
every codebook of the case.  (In the table case, whose classes lie 100 medians apart by themselves, it is another frame of
the stream the file's own frames come from, scaled alike: a foreign frame that large decides every file's class,
whatever its own frames are.)  test_vq_classify_cases_cpu.py asserts on the oracle alone that dropping, doubling or giving away
any planted frame changes the pair's '%g' text.

Seeds: every seed below is the first one tried; none had to be replaced to satisfy those conditions."""
import functools
import os

import numpy as np

import ecoz2rs_amd as e
from tests import oracle_lib

DEFAULT_CHUNK = 1 << 17  # ECOZ2_VQ_QUANTIZE_CHUNK unset
CHUNKS = (None, 1024, 1500)  # the settings the GPU tests run
CUT_CHUNKS = (1024, 1500)  # the settings that cut a file of these cases

# P = 36: every route of e2vq_quantize_device (see ROUTES_36) in an order that is not ascending M, the two M = 256 codebooks
# side by side (a limb image kept across a switch between them would be the other one's), 8224 -> 4096 -> 64 shrinking,
# 300 between two prefiltered sizes, 8192 last and 2048 first (the classify loop goes from the last codebook of a unit to the
# first of the next: the image buffer, grown for 8192, serves 2048 again)
M_ORDER_36 = ("2048", "256", "256b", "8", "8224", "4096", "64", "300", "128", "288", "8192")
ROUTES_36 = {8: "plain", 64: "plain", 128: "plain", 256: "prefiltered", 288: "prefiltered", 300: "plain", 2048: "prefiltered",
             4096: "prefiltered", 8192: "prefiltered", 8224: "plain"}
# at a 1024-frame unit: the first eight fill a unit exactly, 1023 is a unit of its own, 1024 equals the chunk and is not cut,
# 1025 is cut as 1024 + 1, 2500 as 1024 + 1024 + 452; the list ends on an empty file
LENGTHS_36 = (0, 1, 63, 64, 65, 300, 531, 1, 1023, 1024, 1025, 2500, 0)
OTHER_ORDERS = (20, 40, 48, 100)
M_ORDER_OTHER = ("256", "8", "300")
LENGTHS_OTHER = (1, 65, 700, 1025)

# the switching sequence of one session: (codebook, frames); 3000 frames at the third step regrow the fallback list
SWITCH_T = (1, 65, 3000, 700)
SWITCH_36 = ("8", "256", "256b", "256", "4096", "300", "2048", "8192", "8224", "64", "256")
SWITCH_48 = ("8", "256", "256b", "256", "300", "2048", "64", "256")

SEED_CONTINUUM = 20281  # (the stream of test_long_fallback_lists_take_the_wide_sweep)
SEED_CLASSES = 4100  # + P: the class stream of the other orders
SEED_OUTLIER = 977  # + P: the stream the planted frames come from
SEED_TABLE = {"A": 101, "B": 202, "C": 303}  # one prototype per class, as test_vq_classify has them
# the files of the table case: (directory, selection, label, class the frames come from, T)
TABLE_ROWS = (("C", "00000", "C", "C", 300), ("A", "00000", "A", "A", 700), ("A", "00001", "A", "A", 0),
              ("B", "00000", "B", "B", 1025), ("Bdup", "00000", "Bdup", "B", 65), ("E", "00000", "E", "A", 0),
              ("A", "00002", "A", "C", 64), ("C", "00001", "C", "A", 1), ("E", "00001", "E", "B", 0),
              ("B", "00001", "B", "B", 1500))
LENGTHS_TABLE = tuple(r[4] for r in TABLE_ROWS)


def prefiltered(P, M):
    """e2vq_quantize_is_prefiltered restated: a prefilter order, 256 <= M <= 8192, M a multiple of 32"""
    return P in (12, 16, 20, 24, 28, 32, 36, 40) and M >= 256 and M % 32 == 0 and M <= 8192


def chunk_frames(chunk):
    return max(1024, DEFAULT_CHUNK if chunk is None else int(chunk))


def units(Ts, chunk):
    """The unit plan of ecoz2_vq_classify restated: a list of units, each a list of segments (file, t0, n, off) -- short files
    batched (a unit is flushed when the next file would overflow it), a file longer than the chunk cut into units of its
    own.  Empty files stay in the plan as segments of n = 0."""
    chunk = chunk_frames(chunk)
    out, cur, n = [], [], 0
    for k, T in enumerate(Ts):
        if T <= chunk:
            if n + T > chunk:
                if cur:
                    out.append(cur)
                cur, n = [], 0
            cur.append((k, 0, T, n))
            n += T
        else:
            if cur:
                out.append(cur)
            cur, n = [], 0
            for t0 in range(0, T, chunk):
                out.append([(k, t0, min(chunk, T - t0), 0)])
    if cur:
        out.append(cur)
    return out


def planted_places(T, chunks=CUT_CHUNKS):
    """where a file of T frames carries planted frames: both ends, both sides of every cut"""
    if T < 2:
        return []
    at = {0, T - 1}
    for c in chunks:
        if T > c:
            for t0 in range(c, T, c):
                at.update((t0 - 1, t0))
    return sorted(at)


def score(dmin):
    """the classify sum: Python floats, frame order"""
    acc = 0.0
    for d in dmin.tolist():
        acc += d - 1.0
    return acc / len(dmin) if len(dmin) else 0.0


def report(cb_classes, prd_paths, prd_classes, Ts, scores, show_ranked):
    """The exact stdout of ecoz2_vq_classify, restated: scores[k][i] of file k under codebook i."""
    out = []
    classes, ok_by, n_by = [], [], []
    for k, path in enumerate(prd_paths):
        if Ts[k] < 1:
            continue
        sc = scores[k]
        best = 0
        for i in range(1, len(sc)):
            if sc[i] < sc[best]:
                best = i
        ok = cb_classes[best] == prd_classes[k]
        if prd_classes[k] not in classes:
            classes.append(prd_classes[k])
            ok_by.append(0)
            n_by.append(0)
        ci = classes.index(prd_classes[k])
        n_by[ci] += 1
        ok_by[ci] += ok
        if not ok and show_ranked:
            order = sorted(range(len(sc)), key=lambda i: sc[i])  # (stable)
            out.append("%s: '%s' classified as '%s'; ranked:%s\n" % (
                path, prd_classes[k], cb_classes[best], "".join(" %s(%s)" % (cb_classes[i], "%g" % sc[i]) for i in order)))
    out.append("\n%-24s %8s %8s %8s\n" % ("class", "tests", "correct", "percent"))
    for c, n, ok in zip(classes, n_by, ok_by):
        out.append("%-24s %8d %8d %7.2f%%\n" % (c, n, ok, 100.0 * ok / n))
    total, correct = sum(n_by), sum(ok_by)
    out.append("%-24s %8d %8d %7.2f%%\n" % ("TOTAL", total, correct, 100.0 * correct / total if total else 0.0))
    return "".join(out)


# ---- codebooks and frames ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle():
    return oracle_lib.load()


def codebook(src, M, seed):
    """as tests/test_gpu_prefilter.py::_codebook and tools/fuzz_parity.py: the reflections of M synthetic frames, each row
    scaled by a factor in 0.9 ... 1.0"""
    P = src.shape[1] - 1
    rng = np.random.default_rng(seed)
    idx = rng.choice(src.shape[0], size=M, replace=src.shape[0] < M)
    refl = np.zeros((M, P + 1))
    for i, t in enumerate(idx):
        st, _pe, rc, _a = oracle().lpca_r(src[t], P)
        assert st == 0
        refl[i, 1:] = rc[1:] * rng.uniform(0.9, 1.0)
    return refl


def _continuum(P, first, T):
    return e.synth.synth_frames_kind(SEED_CONTINUUM, 1, 6, 0.01, P, first, T)


@functools.lru_cache(maxsize=None)
def size_codebooks(P, kind):
    """name -> reflections, names being sizes ("256b": a second codebook of 256 rows with other contents).  kind
    "continuum": rows drawn from the continuum the P = 36 files and the switching frames come from; "classes": from the
    class stream of the other orders."""
    if kind == "continuum":
        names = dict.fromkeys(SWITCH_48 if P == 48 else M_ORDER_36 + SWITCH_36)
        pool = _continuum(P, 100_000, 12_000)
    else:
        names = M_ORDER_OTHER
        pool = e.synth.synth_frames(SEED_CLASSES + P, 4, P, 100_000, 2_000)
    # (the generator of a codebook's rows and factors is seeded by its order and its name)
    return {name: codebook(pool, int(name.rstrip("b")), 100_000 * P + 2 * int(name.rstrip("b")) + name.endswith("b"))
            for name in names}


class Case:
    """codebooks in call order [(class name, reflections)], files in call order [(dir, selection, label, frames)]"""

    def __init__(self, name, P, cbs, files, planted, tie=()):
        self.name, self.P, self.cbs, self.files, self.planted, self.tie = name, P, cbs, files, planted, tie
        self.Ts = [len(f[3]) for f in files]

    @functools.cached_property
    def dmin(self):
        """dmin[k][i]: the oracle's minimum distortions of file k under codebook i"""
        cqs = [oracle().reflections_to_cq(refl) for _c, refl in self.cbs]
        return [[oracle().quantize(cq, f[3])[1] if len(f[3]) else np.zeros(0) for cq in cqs] for f in self.files]

    @functools.cached_property
    def scores(self):
        return [[score(d) for d in row] for row in self.dmin]

    def write(self, root):
        """-> (codebook paths, predictor paths) in call order, under root/data/{codebooks,predictors}"""
        cbs, prds = [], []
        for cls, refl in self.cbs:
            p = os.path.join(str(root), "data", "codebooks", cls, "eps_0.05_M_%04d.cbook" % len(refl))
            e.formats.write_cbook(p, cls, refl)
            cbs.append(p)
        for d, sel, label, frames in self.files:
            p = os.path.join(str(root), "data", "predictors", d, sel + ".prd")
            e.formats.write_prd(p, label, frames.reshape(-1, self.P + 1))
            prds.append(p)
        return cbs, prds

    def report(self, prd_paths, show_ranked, cb_order=None):
        order = list(range(len(self.cbs))) if cb_order is None else cb_order
        return report([self.cbs[i][0] for i in order], prd_paths, [f[2] for f in self.files], self.Ts,
                      [[row[i] for i in order] for row in self.scores], show_ranked)


def _plant(P, cbs, base, source):
    """base frames of the files -> (frames with the planted ones, planted places per file).  The planted frames of file k are
    source(k, n) times 2^j, j per frame the least that lifts its dmin - 1 to 105 medians of the file's own frames under every
    codebook (a distortion is linear in the frame; the CPU test asserts 100 medians of the file as written)."""
    cqs = [oracle().reflections_to_cq(refl) for refl in cbs]
    out, places = [], []
    for k, fr in enumerate(base):
        at = planted_places(len(fr))
        fr = fr.copy()
        if at:
            x = source(k, len(at))
            need = np.ones(len(at))
            for cq in cqs:
                med = float(np.median(oracle().quantize(cq, fr)[1] - 1.0))
                d1 = oracle().quantize(cq, x)[1]
                need = np.maximum(need, (100.0 * med + 1.0) * 1.05 / d1)
            fr[at] = x * (2.0 ** np.ceil(np.log2(need)))[:, None]
        out.append(fr)
        places.append(at)
    return out, places


@functools.lru_cache(maxsize=None)
def sizes_case(P):
    """the case of the scores tests: every file under a class name no codebook has, so that every (file, codebook) score is
    printed.  P = 36: ROUTES_36 x LENGTHS_36 on the continuum; another order: M = 256, 8, 300 x LENGTHS_OTHER on classes."""
    if P == 36:
        cb, order, lengths = size_codebooks(36, "continuum"), M_ORDER_36, LENGTHS_36
        first = np.cumsum((0,) + lengths[:-1]) + 3 * np.arange(len(lengths))
        base = [_continuum(P, int(a), T) for a, T in zip(first, lengths)]
    else:
        cb, order, lengths = size_codebooks(P, "classes"), M_ORDER_OTHER, LENGTHS_OTHER
        base = [e.synth.synth_frames(SEED_CLASSES + P, 4, P, 2000 * k, T) for k, T in enumerate(lengths)]
    cbs = [("M" + name, cb[name]) for name in order]
    frames, places = _plant(P, [c[1] for c in cbs], base, lambda k, n: e.synth.synth_frames(SEED_OUTLIER + P, 1, P, 16 * k, n))
    files = [("none", "%05d" % k, "none", f) for k, f in enumerate(frames)]
    return Case("sizes%d" % P, P, cbs, files, places)


@functools.lru_cache(maxsize=None)
def table_case():
    """the case of the table tests (P = 36): files under their true labels, a few under wrong ones, two codebooks of identical
    reflections under different class names, an empty file among A's, a class (E) all of whose files are empty, TRAIN rows
    for the CLI's tt list to leave out.  Codebook order of the API tests: C, Bdup, B, A (Bdup wins the tie); the CLI sorts
    the paths: A, B, Bdup, C (B wins it)."""
    P = 36
    src = {c: e.synth.synth_frames(s, 1, P, 0, 4000) for c, s in SEED_TABLE.items()}
    cb = {"A": codebook(src["A"], 64, 11), "B": codebook(src["B"], 256, 12), "C": codebook(src["C"], 8, 13)}
    cbs = [("C", cb["C"]), ("Bdup", cb["B"].copy()), ("B", cb["B"]), ("A", cb["A"])]
    rows = TABLE_ROWS
    base = [e.synth.synth_frames(SEED_TABLE[s], 1, P, 10_000 + 2000 * k, T) for k, (_d, _n, _l, s, T) in enumerate(rows)]
    frames, places = _plant(P, [c[1] for c in cbs], base,
                            lambda k, n: e.synth.synth_frames(SEED_TABLE[rows[k][3]], 1, P, 90_000 + 16 * k, n))
    files = [(d, n, label, f) for (d, n, label, _s, _T), f in zip(rows, frames)]
    return Case("table", P, cbs, files, places, tie=(1, 2))


def case_names():
    return ["sizes36"] + ["sizes%d" % P for P in OTHER_ORDERS] + ["table"]


def case(name):
    return table_case() if name == "table" else sizes_case(int(name[5:]))


# ---- switching in one session --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def switch_steps(P):
    """[(codebook name, reflections, frames, oracle sym, oracle dmin)] of the switching sequence at order P"""
    seq = SWITCH_48 if P == 48 else SWITCH_36
    cb = size_codebooks(P, "continuum")
    pool = _continuum(P, 50_000, max(SWITCH_T))
    steps = []
    for q, name in enumerate(seq):
        frames = np.ascontiguousarray(pool[:SWITCH_T[q % len(SWITCH_T)]])
        sym, dmin = oracle().quantize(oracle().reflections_to_cq(cb[name]), frames)
        steps.append((name, cb[name], frames, sym, dmin))
    return steps
