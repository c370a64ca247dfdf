"""the shared inputs of test_hmm_scan_cpu.py and test_gpu_hmm_scan_shapes.py: a restatement of the
arithmetic by which scan_device (hmm_decode.cpp) cuts the windows into runs and launches (`scan_plan`), held against the
sources by the CPU file; the reference of a scan from the CPU oracle alone (`reference`: H.forward and H.log_prob on every
distinct window, never hmm.score); the rows of SCAN_SHAPES, each at an edge of the staging area, of the run table or of a
launch limit; and the event streams that bring status 1 and status 2 to every position of a window."""
import numpy as np

# ---- the restated constants (test_hmm_scan_cpu.py holds them against hmm_device.h, hmm_scan.hip and hmm_decode.cpp) ----------
WAVE_N = 64
SCAN_SPAN_CAP = 8192
SCAN_WAVES = 4
SCAN_PACK_MAX_N = 21
SCAN_ROUNDS_DEFAULT = 4
SCAN_ROUNDS_MAX = 64
WG_WINDOWS_PER_LAUNCH = 1 << 20
MODELS_PER_LAUNCH = 65535
PACKS = (None, "0", "1")  # ECOZ2_HMM_SCAN_PACK: the host's choice, one window per wave, packed


def _wrap64(x):
    """x as an int64 holds it after two's-complement wrap"""
    return (int(x) + (1 << 63)) % (1 << 64) - (1 << 63)


def _wrap32(x):
    """(int)x of an int64"""
    return (int(x) + (1 << 31)) % (1 << 32) - (1 << 31)


def scan_pack_width_in_use(N, pack=None):
    """windows to a wave; pack: the value of ECOZ2_HMM_SCAN_PACK (None or "": unset)"""
    if pack is not None and pack != "":
        return 1 if int(pack) == 0 or N > 32 else WAVE_N // N
    return WAVE_N // N if N <= SCAN_PACK_MAX_N else 1


def scan_rounds(rounds=None):
    """rounds: the value of ECOZ2_HMM_SCAN_ROUNDS (None: unset); clamped to 1 .. 64"""
    r = SCAN_ROUNDS_DEFAULT if rounds is None else int(rounds)
    return min(max(r, 1), SCAN_ROUNDS_MAX)


def window_counts(lens, window, hop):
    return [(T - window) // hop + 1 if T >= window else 0 for T in lens]


def scan_plan(Ns, lens, window, hop, rounds=SCAN_ROUNDS_DEFAULT, pack=None, formula="runs"):
    """what scan_device launches for models of Ns states over streams of `lens` symbols.  -> dict: W, counts (windows per
    stream), launches {N: dict(G, cap, span_lds, runs = per stream with windows the list of its run counts, lds = bytes of
    dynamic LDS, staged)} for every distinct N <= 64, big = the models of more states, wg_launches = launches of
    k_hmm_scan_wg per 65535 of them.  formula "runs": span_lds from the runs the launch makes; "parent": the earlier
    (min(cap, W) - 1) hop + window in int64, wrap included (the defect the runs' formula replaced)"""
    counts = window_counts(lens, window, hop)
    W = sum(counts)
    launches = {}
    for N in sorted({n for n in Ns if n <= WAVE_N}):
        G = scan_pack_width_in_use(N, pack)
        cap = SCAN_WAVES * G * scan_rounds(rounds)
        if window <= SCAN_SPAN_CAP:
            cap = min(cap, (SCAN_SPAN_CAP - window) // hop + 1)
        runs = [[min(cap, n - w) for w in range(0, n, cap)] for n in counts if n]
        if formula == "runs":
            span = max([(min(cap, n) - 1) * hop + window for n in counts if n], default=0)
            assert span < (1 << 63)  # (no wrap: a run lies within its stream)
        else:
            assert formula == "parent"
            span = _wrap64(_wrap64((min(cap, W) - 1) * hop) + window)
        span_lds = _wrap32(span) if span <= SCAN_SPAN_CAP else 0
        launches[N] = dict(G=G, cap=cap, span_lds=span_lds, runs=runs, lds=N * G * N * 8 + 2 * span_lds,
                           staged=span_lds > 0, refused=span_lds < 0 or span_lds > SCAN_SPAN_CAP)
    big = [k for k, n in enumerate(Ns) if n > WAVE_N]
    wg = -(-W // WG_WINDOWS_PER_LAUNCH) if big else 0
    return dict(W=W, counts=counts, launches=launches, big=big, wg_launches=wg)


def longest_true_span(plan, window, hop):
    """per N the symbols the longest run of the launch covers, (count - 1) hop + window"""
    return {N: max([(c - 1) * hop + window for r in l["runs"] for c in r], default=0) for N, l in plan["launches"].items()}


# ---- models and streams ------------------------------------------------------------------------------------------------------
def model(rng, N, M, zero_cols=()):
    """as test_gpu_hmm_scan.py's _model"""
    row = lambda n: (lambda x: x / x.sum())(rng.uniform(0.05, 1.0, n))
    pi, A, B = row(N), np.stack([row(N) for _ in range(N)]), np.stack([row(M) for _ in range(N)])
    for c in zero_cols:
        B[:, c] = 0.0
    return pi, A, B


HUGE_HOPS = (8, 1 << 40, 1 << 62, (1 << 63) - 1)

# name: (N of the models, M, stream lengths, window, hops)
SCAN_SHAPES = {
    "L8192": ((64, 64, 5), 16, (100, 8192, 0, 8193), 8192, (1,)),         # a window of exactly the staging area
    "L8191": ((64, 21), 16, (7, 8193), 8191, (1,)),                       # a run of two windows whose span is exactly 8192
    "L8193": ((64, 22, 5), 16, (7, 8200, 8193), 8193, (1,)),              # one symbol too long: k_hmm_scan<false>
    "L4000_H1000": ((64, 16, 5), 16, (3999, 16000, 9000), 4000, (1000,)),  # the span rule cuts the runs at every N
    "rounds_N1": ((1, 1), 16, (9000,), 37, (1,)),
    "rounds_N21_N64": ((21, 64), 16, (1500,), 37, (1,)),
    "many_windows": ((3, 65), 4, ((1 << 20) + 5,), 2, (1,)),               # a second launch of k_hmm_scan_wg
    "huge_hop_long": ((5, 64), 16, (8193, 8200, 8193), 8193, HUGE_HOPS),
    "huge_hop_short": ((5, 64), 16, (100, 150, 100), 100, HUGE_HOPS),
}
MANY_HEAD, MANY_TAIL = (3, 3, 1, 0, 2), (0, 1, 3, 2, 0)  # the first and the last four windows: eight different pairs

_shapes = {}


def scan_shape(name):
    """-> (models, streams, window, hops) of a row; the same arrays at every call"""
    if name not in _shapes:
        Ns, M, lens, L, hops = SCAN_SHAPES[name]
        rng = np.random.default_rng(sorted(SCAN_SHAPES).index(name) + 4850)
        models = [model(rng, N, M) for N in Ns]
        streams = [rng.integers(0, M, n).astype(np.uint16) for n in lens]
        if name == "many_windows":
            streams[0][:5], streams[0][-5:] = MANY_HEAD, MANY_TAIL
        for s in streams:
            s.setflags(write=False)
        _shapes[name] = (models, streams, L, hops)
    return _shapes[name]


# ---- the reference: the CPU oracle on every distinct window ------------------------------------------------------------------
def windows_of(streams, window, hop):
    """-> (win_offs, [(stream, first)] of every window)"""
    counts = window_counts([len(s) for s in streams], window, hop)
    at = [(s, i * hop) for s, n in enumerate(counts) for i in range(n)]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), at


def rank(status, exp2, mant):
    """best and second model of every window on (status == 0, exp2, mant), the later model first among equals
    (k_scan_top2's contract); a status other than 0 is P = 0.  second is -1 with one model"""
    v = status == 0
    e, m = np.where(v, exp2, 0), np.where(v, mant, 0.0)
    k = np.broadcast_to(np.arange(status.shape[1]), status.shape)
    order = np.lexsort((k, m, e, v), axis=1)  # ascending; the last key counts most
    best = order[:, -1].astype(np.int32)
    second = order[:, -2].astype(np.int32) if status.shape[1] > 1 else np.full(len(status), -1, np.int32)
    return best, second


def reference(H, models, streams, window, hop):
    """the scan's results from the oracle: win_offs, the W x K mant / exp2 / status / log_prob, best / second and their
    log-probabilities.  One oracle call per model and distinct window (by the window's bytes)."""
    win_offs, at = windows_of(streams, window, hop)
    K = len(models)
    seen, inv, uniq = {}, np.zeros(len(at), np.int64), []
    if window * 2 <= 8 and len(at) > 4096:  # short windows in great number: their keys at once
        keys = np.concatenate([sum(s[j:len(s) - window + 1 + j].astype(np.uint64) << np.uint64(16 * j) for j in range(window))[::hop]
                               for s, n in zip(streams, np.diff(win_offs)) if n])
        vals, first, inv = np.unique(keys, return_index=True, return_inverse=True)
        uniq = [at[i] for i in first]
    else:
        for w, (s, i) in enumerate(at):
            key = streams[s][i:i + window].tobytes()
            if key not in seen:
                seen[key] = len(uniq)
                uniq.append((s, i))
            inv[w] = seen[key]
    U = len(uniq)
    mant, exp2 = np.zeros((U, K)), np.zeros((U, K), np.int64)
    status, lp = np.zeros((U, K), np.int32), np.zeros((U, K))
    for u, (s, i) in enumerate(uniq):
        sym = streams[s][i:i + window]
        for k, (pi, A, B) in enumerate(models):
            st, m, e = H.forward(pi, A, B, sym)
            if st != 0:
                m, e = 0.0, 0
            status[u, k], mant[u, k], exp2[u, k], lp[u, k] = st, m, e, H.log_prob(m, e)
    out = dict(win_offs=win_offs, mant=mant[inv], exp2=exp2[inv], status=status[inv], log_prob=lp[inv], oracle_calls=U * K)
    best, second = rank(out["status"], out["exp2"], out["mant"])
    rows = np.arange(len(at))
    out["best"], out["second"] = best, second
    out["best_log_prob"] = out["log_prob"][rows, best] if len(at) else np.zeros(0)
    out["second_log_prob"] = out["log_prob"][rows, second] if K > 1 and len(at) else np.full(len(at), -np.inf)
    return out


_refs = {}


def shape_reference(H, name, hop):
    """the reference of a row at one of its hops, computed once"""
    if (name, hop) not in _refs:
        models, streams, L, hops = scan_shape(name)
        assert hop in hops
        _refs[name, hop] = reference(H, models, streams, L, hop)
    return _refs[name, hop]


# ---- events: a symbol outside the alphabet (status 2) and one no state can emit (status 1) at every position -----------------
EVENT_NS = (5, 22, 64, 70)
EVENT_M, EVENT_L, EVENT_H = 16, 37, 1
EVENT_LENS = (60, 300)      # one short clean stream, then the stream that takes the events
EVENT_AT = (0, 150, 299)    # the first symbol, the middle, the last symbol
EVENT_OUTSIDE = EVENT_M + 9
EVENT_DEAD = 11             # its column of B is zero in every model of the "dead" cases
EVENT_KINDS = ("outside", "dead")
EVENT_STATUS = {"outside": 2, "dead": 1}
UNSTAGED_EVENT_AT = (3, 8199)  # of the 8200 symbols of row L8193's second stream

_events = {}


def _without_dead(stream, M):
    s = stream.copy()
    s[s == EVENT_DEAD] = (EVENT_DEAD + 1) % M
    return s


def _plant(streams, which, at, symbol):
    dirty = [s.copy() for s in streams]
    dirty[which][list(at)] = symbol
    return dirty


def events_case(kind):
    """-> (models, clean streams, dirty streams, window, hop): N = 5, 22, 64 and 70 over a short clean stream and one of 300
    symbols with the event symbol at EVENT_AT.  No clean symbol is EVENT_DEAD (in either kind: the streams are the same)"""
    if kind not in _events:
        rng = np.random.default_rng(4851 + EVENT_KINDS.index(kind))
        models = [model(rng, N, EVENT_M, zero_cols=(EVENT_DEAD,) if kind == "dead" else ()) for N in EVENT_NS]
        srng = np.random.default_rng(4853)
        clean = [_without_dead(srng.integers(0, EVENT_M, n).astype(np.uint16), EVENT_M) for n in EVENT_LENS]
        dirty = _plant(clean, 1, EVENT_AT, EVENT_OUTSIDE if kind == "outside" else EVENT_DEAD)
        _events[kind] = (models, clean, dirty, EVENT_L, EVENT_H)
    return _events[kind]


def unstaged_events_case(kind):
    """row L8193's streams and N with the event symbol at indices 3 and 8199 of the 8200-symbol stream: windows 0 .. 3 are
    hit at t = 3 .. 0, window 7 at t = 8192, windows 4 .. 6 and the third stream's window are clean"""
    key = ("unstaged", kind)
    if key not in _events:
        Ns, M, _lens, L, (H,) = SCAN_SHAPES["L8193"]
        _models, streams, _L, _hops = scan_shape("L8193")
        if kind == "dead":
            rng = np.random.default_rng(4855)
            models = [model(rng, N, M, zero_cols=(EVENT_DEAD,)) for N in Ns]
            clean = [_without_dead(s, M) for s in streams]
        else:
            models, clean = _models, [s.copy() for s in streams]
        dirty = _plant(clean, 1, UNSTAGED_EVENT_AT, EVENT_OUTSIDE if kind == "outside" else EVENT_DEAD)
        _events[key] = (models, clean, dirty, L, H)
    return _events[key]


def hits(streams_lens, window, hop, which, at):
    """per window the positions t at which a symbol planted at the indices `at` of stream `which` lies (a list, maybe empty)"""
    out = []
    for s, n in enumerate(window_counts(streams_lens, window, hop)):
        for i in range(n):
            out.append([p - i * hop for p in at if s == which and i * hop <= p < i * hop + window])
    return out
