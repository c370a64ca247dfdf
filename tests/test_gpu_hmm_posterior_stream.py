"""`hmm segment --continuous-posteriors` on the GPU: the rows a posterior session delivers against the
restatement and against e2vq_hmm_segment_posteriors on the prefixes, bit for bit, for both bodies, A in LDS and in global
memory, ring lengths that are and are not multiples of 64, and four feed patterns; the stream-length edges; a ring that wraps;
device memory that does not grow; the closed pass at L >= T; the status rules at the edges of the hand-out, of a block, of the
look-ahead and of the remainder; the file form and the CLI against `--posteriors` and `--continuous`; a device tensor."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_class_loop_cases as loop_cases
from . import hmm_posterior_stream_restatement as RS
from .hmm_posterior_looped_cases import posteriors_one  # (the closed restatement without its cap of 16 slots)
from .test_hmm_segment_stream_cpu import planted_models, planted_stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
NINF = float("-inf")
BODY = "ECOZ2_HMM_POSTERIOR_BODY"
LS = loop_cases.EVENT_LN_SWITCH
M, DEAD = loop_cases.EVENT_M, loop_cases.DEAD
T, B = 300, 64
LOOKAHEADS = (0, 1, 63, 64, 100)  # B + L = 64, 65, 127, 128, 164
# name: (N of every class, body).  Dense models no state of which emits DEAD (hmm_class_loop_cases).
PACKINGS = {
    "5_3_4": ((5, 3, 4), None),                   # resident, one slot, A in LDS
    "21_22_64": ((21, 22, 64), "resident"),       # resident: a packed slot (ds_bpermute chains) next to a one-class slot (v_readlane)
    "64x5": ((64,) * 5, None),                    # resident, A (166 KB) in global memory
    "5_3_4/looped": ((5, 3, 4), "looped"),        # the looped body forced below 17 slots, A in LDS
    "64x5/looped": ((64,) * 5, "looped"),         # the same with A in global memory
    "33x17/auto": ((33,) * 17, "auto"),           # 17 slots: looped under auto, wave 0 serves two slots; A (145 KB) in LDS
}


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture(autouse=True)
def _no_body(monkeypatch):
    monkeypatch.delenv(BODY, raising=False)


def _clean(n, seed=130):
    return np.random.default_rng(seed).integers(0, DEAD, n).astype(np.uint16)


_MODELS, _CACHES = {}, {}


def _case(name):
    """-> (models, body, the cache of the closed restatement on the prefixes of _clean(T)): computed once, shared, read only"""
    Ns, body = PACKINGS[name]
    if Ns not in _MODELS:
        _MODELS[Ns] = loop_cases.align_cases.event_models(Ns)
        _CACHES[Ns] = {}
    return _MODELS[Ns], body, _CACHES[Ns]


def _feeds(n, sizes):
    out = []
    while sum(out) < n:
        out.append(min(sizes[len(out) % len(sizes)], n - sum(out)))
    return out


def _session(models, sym, B_, L, feeds, body=None, ls=LS, want_ready=None):
    """a session fed sym in pieces of the lengths `feeds` and closed -> dict post (every row), ready (after each feed),
    log_prob, status, stats"""
    parts, ready, at = [], [], 0
    with hmm.PosteriorStream(models, ls, block=B_, lookahead=L, body=body) as s:
        for n in feeds:
            first, rows = s.feed(sym[at:at + n])
            at += n
            assert first == sum(len(p) for p in parts) and first + len(rows) == s.ready_frames
            if want_ready is not None:
                assert s.ready_frames == want_ready(at), (at, s.ready_frames)
            parts.append(rows)
            ready.append(s.ready_frames)
        first, rows = s.close()
        parts.append(rows)
        assert s.ready_frames == len(sym) == first + len(rows)
        return dict(post=np.concatenate(parts), ready=ready, log_prob=s.log_prob, status=s.status, stats=s.stats(), kernel_ms=s.kernel_ms())


# ---- bits against the restatement and the closed GPU pass ---------------------------------------------------------------------
@pytest.mark.parametrize("L", LOOKAHEADS)
@pytest.mark.parametrize("name", list(PACKINGS))
def test_rows_are_the_closed_pass_on_the_prefix_bit_for_bit(name, L):
    models, body, cache = _case(name)
    sym = _clean(T)
    want, _ready, rows = RS.run(models, sym, LS, B, L, [T], closed_pass=posteriors_one, cache=cache)
    assert want.status == 0 and rows.shape == (T, len(models))
    # the closed GPU pass on every prefix a window ends at, in one call
    ends = sorted({min(want.window_end(b), T) for b in range((T + B - 1) // B)})
    offs = np.concatenate([[0], np.cumsum(ends)]).astype(np.int64)
    closed = hmm.segment_posteriors(models, np.concatenate([sym[:w] for w in ends]), offs, LS, body=body)
    assert not closed["status"].any()
    for t0 in range(0, T, B):
        i = ends.index(min(want.window_end(t0 // B), T))
        assert _same(rows[t0:t0 + B], closed["post"][offs[i] + t0:offs[i] + min(t0 + B, T)]), (name, L, t0)
    for pattern in ([T], _feeds(T, (B,)), _feeds(T, (63, 64, 65))):
        got = _session(models, sym, B, L, pattern, body=body, want_ready=want.ready_after)
        assert _same(got["post"], rows), (name, L, pattern[:3])
        assert got["status"] == 0 and _bits(got["log_prob"]) == _bits(want.log_prob) == _bits(closed["log_prob"][-1])
        assert got["stats"]["ring_rows"] == B + L and got["stats"]["launches"] == want.launches
        assert got["stats"]["backward_frames"] == want.walked and got["kernel_ms"] > 0.0


@pytest.mark.parametrize("name,L", [("5_3_4", 1), ("5_3_4/looped", 63)])
def test_symbol_by_symbol(name, L):
    models, body, cache = _case(name)
    sym = _clean(T)
    want, _ready, rows = RS.run(models, sym, LS, B, L, [T], closed_pass=posteriors_one, cache=cache)
    got = _session(models, sym, B, L, [1] * T, body=body, want_ready=want.ready_after)
    assert _same(got["post"], rows) and _bits(got["log_prob"]) == _bits(want.log_prob)


# ---- the edges of the stream's length, a ring that wraps, memory -----------------------------------------------------------------
@pytest.mark.parametrize("body", ["resident", "looped"])
@pytest.mark.parametrize("n,B_,L", [(0, 64, 10), (1, 64, 0), (40, 64, 10), (64, 64, 0), (64, 64, 10), (138, 64, 10), (202, 64, 10), (65, 1, 0)])
def test_stream_length_edges(n, B_, L, body):
    """T = 0; T < B (only close delivers); T = B; T = (b + 1) B + L exactly (the last feed delivers block b, close the L
    frames behind it without a forward step); B = 1 and L = 0 (a ring of one row)"""
    models = _case("5_3_4")[0]
    sym = _clean(n, seed=7)
    want, ready, rows = RS.run(models, sym, LS, B_, L, [n] if n else [], closed_pass=posteriors_one)
    for feeds in ([n] if n else [], _feeds(n, (33,))):
        got = _session(models, sym, B_, L, feeds, body=body, want_ready=want.ready_after)
        assert _same(got["post"], rows.reshape(n, 3)) and got["status"] == 0 and _bits(got["log_prob"]) == _bits(want.log_prob)
        assert got["stats"]["launches"] == want.launches
    if n == 0:
        assert got["log_prob"] == 0.0 and got["post"].shape == (0, 3) and got["stats"]["launches"] == 0
    if n < B_:
        assert ready in ([], [0]) and want.launches == (1 if n else 0)
    if n == 138:
        assert ready == [128] and want.launches == 3 and want.walked == 2 * 74 + 10


@pytest.mark.parametrize("name", ["21_22_64", "64x5/looped"])
def test_the_ring_wraps(name):
    """B + L = 11 rows and 3 x 11 + 8 frames: every row is written four times, no chunk of 64 symbols lies in the ring unbroken"""
    models, body, _cache = _case(name)
    sym = _clean(41, seed=11)
    want, _ready, rows = RS.run(models, sym, LS, 7, 4, [41], closed_pass=posteriors_one)
    for feeds in ([41], _feeds(41, (5, 9))):
        got = _session(models, sym, 7, 4, feeds, body=body, want_ready=want.ready_after)
        assert _same(got["post"], rows) and _bits(got["log_prob"]) == _bits(want.log_prob)
    assert got["stats"]["ring_rows"] == 11


def test_device_memory_does_not_grow():
    models = _case("5_3_4")[0]
    B_, L = 16, 9
    sym = _clean(10 * (B_ + L) + 3, seed=3)
    with hmm.PosteriorStream(models, LS, block=B_, lookahead=L) as s:
        before = s.stats()
        for a in range(0, len(sym), 40):
            s.feed(sym[a:a + 40])
        after = s.stats()
        s.close()
        assert s.stats()["device_bytes"] == after["device_bytes"] == before["device_bytes"] > 0
        assert before["ring_rows"] == after["ring_rows"] == B_ + L and before["launches"] == 0 and after["launches"] == (len(sym) - L) // B_
        # 8 (sum N + a wave + K) + 2 bytes a ring row, next to the parameters
        assert before["device_bytes"] >= (B_ + L) * (8 * (12 + 1 + 3) + 2)


def test_a_ring_that_cannot_be_allocated_is_refused_with_its_bytes():
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.PosteriorStream(_case("5_3_4")[0], LS, block=1 << 36, lookahead=5)
    rows = (1 << 36) + 5
    assert f"no room for the ring of {rows} frames x 12 states ({rows * 130} bytes: block {1 << 36} + look-ahead 5)" in str(ei.value)


# ---- L >= T: the closed pass -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PACKINGS))
def test_a_look_ahead_of_the_whole_stream_is_the_closed_pass(name):
    models, body, _cache = _case(name)
    sym = _clean(T)
    closed = hmm.segment_posteriors(models, sym, [0, T], LS, body=body)
    for B_, L, feeds in ((64, T, [T]), (4096, 4096, _feeds(T, (63, 64, 65))), (7, T + 1, _feeds(T, (100,)))):
        got = _session(models, sym, B_, L, feeds, body=body)
        assert got["ready"] == [0] * len(feeds) and got["stats"]["launches"] == 1
        assert _same(got["post"], closed["post"]) and _bits(got["log_prob"]) == _bits(closed["log_prob"][0])
        assert got["status"] == closed["status"][0] == 0


# ---- events ------------------------------------------------------------------------------------------------------------------------
EV_B, EV_L, EV_T = 100, 30, 250  # windows end at 130 and 230; close serves the blocks from 200 on and forwards [230, 250)
EV_AT = (0, 63, 64, 99, 100, 115, 229, 240)  # hand-out edges, B - 1, B, inside a look-ahead, a window's last frame, the remainder


def _script(models, sym, feeds, closed_pass=posteriors_one):
    """what every call of a session does, as the restatement states it -> [(kind, outcome)] per feed and for close:
    outcome = ("rows", first, rows) | ("bad", frame) | ("refused",)"""
    s = RS.Stream(models, LS, EV_B, EV_L, closed_pass=closed_pass)
    log, at = [], 0

    def call(fn, *args):
        try:
            first, rows = fn(*args)
            return ("rows", first, rows)
        except RS.BadSymbol as ex:
            return ("bad", ex.frame)
        except RS.Refused:
            return ("refused",)

    for n in feeds:
        log.append(call(s.feed, sym[at:at + n]))
        at += n
    log.append(call(s.close))
    return s, log


@pytest.mark.parametrize("body", ["resident", "looped"])
@pytest.mark.parametrize("at", EV_AT)
@pytest.mark.parametrize("kind", ["M", "dead"])
def test_events_decide_what_every_call_returns(kind, at, body):
    models = _case("5_3_4")[0]
    feeds = _feeds(EV_T, (70, 60))
    # a clean stream through the same kind of session first: what the allocator hands out again holds non-zero rows
    clean = _session(models, _clean(EV_T), EV_B, EV_L, feeds, body=body)
    assert clean["status"] == 0 and clean["post"].all()
    sym = _clean(EV_T)
    sym[at] = M if kind == "M" else DEAD
    want, log = _script(models, sym, feeds)
    assert (want.status, want.frame) == (2 if kind == "M" else 1, at)
    got_rows = []
    with hmm.PosteriorStream(models, LS, block=EV_B, lookahead=EV_L, body=body) as s:
        a = 0
        for n, step in zip(feeds, log):
            if step[0] == "rows":
                first, rows = s.feed(sym[a:a + n])
                assert first == step[1] and _same(rows, step[2].reshape(len(step[2]), 3))
                got_rows.append(rows)
            else:
                with pytest.raises(e.Ecoz2Error) as ei:
                    s.feed(sym[a:a + n])
                if step[0] == "bad":
                    assert f"e2vq_hmm_posterior_stream_feed: the symbol at frame {at} is outside the models' alphabet of {M}" in str(ei.value)
                else:
                    assert f"met a symbol outside the alphabet at frame {at} and takes no more symbols" in str(ei.value)
            a += n
        step = log[-1]
        if step[0] == "rows":
            first, rows = s.close()
        else:
            assert step == ("bad", at)
            with pytest.raises(e.Ecoz2Error) as ei:
                s.close()
            assert f"e2vq_hmm_posterior_stream_close: the symbol at frame {at} is outside the models' alphabet" in str(ei.value)
            first, rows = s.take()
        got_rows.append(rows)
        assert (s.status, s.log_prob, s.ready_frames) == (want.status, NINF, want.fed)  # (a refused feed is not counted)
        with pytest.raises(e.Ecoz2Error) as ei:
            s.feed(sym[:1])
        assert "the session is closed" in str(ei.value)
    every = np.concatenate(got_rows)
    delivered = RS.ready_after(at, EV_B, EV_L)
    assert _same(every, np.array(want.rows).reshape(want.fed, 3))
    assert _same(every[:delivered], clean["post"][:delivered]) and delivered == (0 if at < 130 else 100 if at < 230 else 200)
    assert not every[delivered:].any() and not np.signbit(every[delivered:]).any()


def test_the_earlier_event_wins_and_the_symbol_check_comes_first():
    models = _case("5_3_4")[0]
    for pair, status, frame in (((DEAD, M), 1, 63), ((M, DEAD), 2, 63)):
        sym = _clean(EV_T)
        sym[63], sym[64] = pair
        with hmm.PosteriorStream(models, LS, block=EV_B, lookahead=EV_L) as s:
            if status == 2:
                with pytest.raises(e.Ecoz2Error) as ei:
                    s.feed(sym)
                assert f"frame {frame} " in str(ei.value)
            else:
                assert s.feed(sym)[1].shape == (0, 3)
                assert s.feed(sym[:40])[1].shape == (0, 3)  # accepted, counted, and nothing else
            first, rows = s.close()
            assert (s.status, s.log_prob, first) == (status, NINF, 0)
            assert rows.shape == (EV_T + (40 if status == 1 else 0), 3) and not rows.any()


# ---- refusals of a live session ---------------------------------------------------------------------------------------------------
def test_feed_and_close_after_close_are_refused():
    with hmm.PosteriorStream(_case("5_3_4")[0], LS, block=8, lookahead=3) as s:
        s.feed(_clean(20))
        s.close()
        for call in (lambda: s.feed(_clean(4)), s.close):
            with pytest.raises(e.Ecoz2Error) as ei:
                call()
            assert "the session is closed" in str(ei.value)
        assert s.take()[1].shape == (0, 3) and s.status == 0


def test_entry_points():
    for name in ("open", "feed", "close", "take", "kernel_ms", "stats", "free"):
        assert hasattr(e.lib, "e2vq_hmm_posterior_stream_" + name)
    assert hasattr(e.lib, "e2vq_hmm_segment_continuous_files_posteriors") and callable(hmm.PosteriorStream)


# ---- a device tensor ---------------------------------------------------------------------------------------------------------------
_TORCH_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
torch.cuda.init()  # (torch first: it has to find the device before the library opens it)
from ecoz2rs_amd import hmm
d = np.load(sys.argv[2])
models = list(zip(d["pi"], d["A"], d["B"]))
dev = torch.from_numpy(d["sym"].view(np.int16)).to("cuda:0")
torch.cuda.synchronize()
parts = []
with hmm.PosteriorStream(models, -3.0, block=64, lookahead=36) as s:
    for a in range(0, len(dev), 90):
        parts.append(s.feed(dev[a:a + 90])[1])
    parts.append(s.close()[1])
    np.savez(sys.argv[3], log_prob=s.log_prob, status=s.status, post=np.concatenate(parts))
print("ok")
"""


def test_symbols_in_a_device_tensor(tmp_path):
    e.hmm.set_random_seed(3)
    models = [hmm.init_model(5, 64, 0) for _ in range(3)]
    sym = np.random.default_rng(9).integers(0, 64, 400).astype(np.uint16)
    want = _session(models, sym, 64, 36, [400], ls=-3.0)
    np.savez(tmp_path / "in.npz", pi=np.stack([m[0] for m in models]), A=np.stack([m[1] for m in models]),
             B=np.stack([m[2] for m in models]), sym=sym)
    r = subprocess.run([sys.executable, "-c", _TORCH_SCRIPT, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
    got = np.load(tmp_path / "out.npz")
    assert _same(got["post"], want["post"]) and _bits(got["log_prob"]) == _bits(want["log_prob"]) and got["status"] == 0


# ---- files and CLI -----------------------------------------------------------------------------------------------------------------
def test_files_equal_the_posteriors_of_the_concatenated_recording(tmp_path):
    env = dict(os.environ)
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_GPUS", "ECOZ2_HMM_SEGMENT_BODY", "ECOZ2_HMM_SEGMENT_CHUNK_BYTES", BODY,
              "ECOZ2_HMM_SEGMENT_STREAM_PENDING_BYTES", "ECOZ2_HMM_POSTERIOR_CHUNK_BYTES"):
        env.pop(k, None)
    env["ECOZ2_HMM_SEGMENT_STREAM_BLOCK"] = "64"
    P, M_, ls = 4, 16, -5.0
    models = planted_models()
    names = ["a", "b", "c"]
    for c, m in zip(names, models):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)
    sym = planted_stream(models, np.random.default_rng(3))
    n = len(sym)
    cuts = [0, 170, 171, n]  # (a piece of one frame among them)
    (tmp_path / "seq").mkdir()
    for i in range(3):
        e.formats.write_seq(str(tmp_path / "seq" / f"p{i}.seq"), "_", M_, sym[cuts[i]:cuts[i + 1]])
    e.formats.write_seq(str(tmp_path / "rec.seq"), "_", M_, sym)
    rng = np.random.default_rng(5)
    e.formats.write_cbook(str(tmp_path / "cb.cbook"), "_", np.hstack([np.zeros((M_, 1)), rng.uniform(-0.8, 0.8, (M_, P))]))
    prd = np.hstack([np.ones((400, 1)), rng.uniform(-0.5, 0.5, (400, P))])
    pcuts = [0, 130, 300, 400]
    (tmp_path / "prd").mkdir()
    for i in range(3):
        e.formats.write_prd(str(tmp_path / "prd" / f"p{i}.prd"), "_", prd[pcuts[i]:pcuts[i + 1]])
    e.formats.write_prd(str(tmp_path / "rec.prd"), "_", prd)

    def run(*args):
        r = subprocess.run([EXE, "hmm", "segment", "--models", "hmms", "--switch-penalty", str(ls), "-P", str(P), *args], cwd=tmp_path,
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout, r.stderr)
        return r.stdout

    def block_of(text, name):
        lines = text.split("\n")
        at = [i for i, l in enumerate(lines) if l.startswith(name + ": T=")]
        assert len(at) == 1, text
        return [l for l in lines[at[0]:] if l and not l.endswith(" saved")]

    for kind, flag, ext, extra, length in (("seq", "--sequences", ".seq", [], n), ("prd", "--predictors", ".prd", ["--codebook", "cb.cbook"], 400)):
        pieces = [f"{kind}/p{i}{ext}" for i in range(3)]
        whole = run(*extra, "-c", f"one_{kind}", "--posteriors", "--frame-posteriors", f"one_{kind}_frames", flag, f"rec{ext}")
        parts = run(*extra, "-c", f"cont_{kind}", "--continuous-posteriors", "rec", "--block", "64", "--lookahead", str(length),
                    "--frame-posteriors", f"cont_{kind}_frames", flag, *pieces)
        want = (tmp_path / f"one_{kind}" / "rec.csv").read_bytes()
        assert (tmp_path / f"cont_{kind}" / "rec.csv").read_bytes() == want and want.count(b"\n") > 3
        assert want.startswith(b"segment,begin_frame,end_frame,begin_s,end_s,class,log_prob,log_prob_per_frame,posterior,min_posterior\n")
        frames = (tmp_path / f"one_{kind}_frames" / "rec.csv").read_bytes()
        assert (tmp_path / f"cont_{kind}_frames" / "rec.csv").read_bytes() == frames and frames.count(b"\n") == length + 1
        assert sorted(os.listdir(tmp_path / f"cont_{kind}")) == sorted(os.listdir(tmp_path / f"cont_{kind}_frames")) == ["rec.csv"]
        b1, b2 = block_of(whole, f"rec{ext}"), block_of(parts, "rec")
        assert b2[0] == "rec" + b1[0][len(f"rec{ext}"):] and b2[1:] == b1[1:] and any(" p=" in l for l in b2)
        # a short look-ahead: the decode is --continuous', the last two columns alone may move; the looped body changes nothing
        run(*extra, "-c", f"plain_{kind}", "--continuous", "rec", flag, *pieces)
        run(*extra, "-c", f"short_{kind}", "--continuous-posteriors", "rec", "--block", "64", "--lookahead", "16", flag, *pieces)
        run(*extra, "-c", f"short_looped_{kind}", "--continuous-posteriors", "rec", "--block", "64", "--lookahead", "16", "--body", "looped",
            flag, *pieces)
        plain = (tmp_path / f"plain_{kind}" / "rec.csv").read_text().splitlines()
        short = (tmp_path / f"short_{kind}" / "rec.csv").read_text().splitlines()
        assert [l.split(",")[:8] for l in short] == [l.split(",") for l in plain] and all(len(l.split(",")) == 10 for l in short)
        assert (tmp_path / f"short_looped_{kind}" / "rec.csv").read_text().splitlines() == short
    # the Python mirror of the file form
    hmm_files = [str(tmp_path / "hmms" / f"{c}.hmm") for c in names]
    os.environ["ECOZ2_HMM_SEGMENT_STREAM_BLOCK"] = "64"
    try:
        hmm.segment_files(hmm_files, [str(tmp_path / "seq" / f"p{i}.seq") for i in range(3)], ls, P=P, csv=tmp_path / "py",
                          frame_posteriors=tmp_path / "py_frames", continuous_posteriors="rec", block=64, lookahead=n)
    finally:
        del os.environ["ECOZ2_HMM_SEGMENT_STREAM_BLOCK"]
    assert (tmp_path / "py" / "rec.csv").read_bytes() == (tmp_path / "one_seq" / "rec.csv").read_bytes()
    assert (tmp_path / "py_frames" / "rec.csv").read_bytes() == (tmp_path / "one_seq_frames" / "rec.csv").read_bytes()
