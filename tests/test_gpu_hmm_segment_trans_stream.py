"""`hmm segment --class-transitions --grammar-continuous` on the GPU: the matrix session against
e2vq_hmm_segment_trans on the concatenation and against the restatement, bit for bit, for every LDS layout, block length, stream
length, feed pattern and kind of price matrix; the frames it delivers after every feed against the restatement's finality
rule; the ring; the status rules; the file form and the CLI against `hmm segment --class-transitions` on the concatenated
file; the Python mirror's segments."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_segment_trans_cases as cases
from . import hmm_segment_trans_stream_restatement as ST
from . import hmm_viterbi_restatement as V
from .test_hmm_segment_stream_cpu import planted_models, planted_stream
from .test_hmm_segment_trans_stream_cpu import planted_prices

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
NINF = float("-inf")
ENV_BLOCK = "ECOZ2_HMM_SEGMENT_STREAM_BLOCK"
ENV_PENDING = "ECOZ2_HMM_SEGMENT_STREAM_PENDING_BYTES"
KEYS = ("cls", "state", "entered", "exit_score")


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _init_models(Ns, M, mtype=0, seed=5):
    e.hmm.set_random_seed(seed)
    return [hmm.init_model(N, M, mtype) for N in Ns]


@pytest.fixture
def block(monkeypatch):
    """sets the block length (and a pending budget: the default ring of 256 MiB is not needed here)"""
    for k in ("ECOZ2_HMM_SEGMENT_BODY", ENV_BLOCK, ENV_PENDING):
        monkeypatch.delenv(k, raising=False)

    def set_block(B, pending=16 << 20):
        monkeypatch.setenv(ENV_BLOCK, str(B))
        monkeypatch.setenv(ENV_PENDING, str(pending))
    set_block(64)
    return set_block


def _stream(models, sym, lt, feeds, on_feed=None, cls=None):
    """the session fed sym in pieces of the lengths `feeds`, closed -> dict of all frames, log_prob, status, finals"""
    parts, finals, at = [], [], 0
    keys = KEYS if cls is None else ("cls", "state", "entered", "gbest")
    with (cls or hmm.SegmentTransStream)(models, lt) as s:
        for n in feeds:
            parts.append(s.feed(sym[at:at + n]))
            at += n
            finals.append(s.final_frames)
            if on_feed:
                on_feed(s, at, parts)
        assert at == len(sym)
        parts.append(s.close())
        out = {k: np.concatenate([p[k] for p in parts]) for k in keys}
        at = 0
        for p in parts:  # (the frames come in order, each once)
            assert p["first"] == at or len(p["cls"]) == 0
            at += len(p["cls"])
        out.update(log_prob=s.log_prob, status=s.status, finals=finals, total=s.final_frames,
                   segments=[g for p in parts for g in p["segments"]], kernel_ms=s.kernel_ms(), stats=s.stats())
    return out


def _assert_one_shot(got, want, note=None):
    for k in KEYS:
        assert _same(got[k], want[k]), (k, note)
    assert _bits(np.float64(got["log_prob"])) == _bits(want["log_prob"])[0] and got["status"] == want["status"][0], note
    assert got["total"] == len(want["cls"])


def _assert_restatement(got, rest, note=None):
    assert rest.join_failures == 0
    assert got["cls"].tolist() == rest.cls and got["state"].tolist() == rest.state and got["entered"].tolist() == rest.entered, note
    assert _same(got["exit_score"], np.array(rest.exit_score, dtype=np.float64)), note
    assert _bits(np.float64(got["log_prob"])) == _bits(np.float64(rest.log_prob)) and got["status"] == rest.status, note


def _patterns(T, B):
    """whole; in whole blocks; as 63, 64, 65 in turn; symbol by symbol (T <= 130)"""
    cyc, i = [], 0
    while sum(cyc) < T:
        cyc.append(min((63, 64, 65)[i % 3], T - sum(cyc)))
        i += 1
    out = {"whole": [T], "blocks": [B] * (T // B) + [T % B], "63_64_65": cyc}
    if T <= 130:
        out["single"] = [1] * T
    return out


# ---- equality with e2vq_hmm_segment_trans and with the restatement ----------------------------------------------------------------
PACKINGS = {
    "1": [1],
    "5": [5],
    "5x3": [5] * 3,
    "5x13": [5] * 13,          # two packed slots
    "21_22_64": [21, 22, 64],  # classes of different N side by side, and a slot of one class
    "64x16": [64] * 16,        # 16 slots, lA from global memory
    "1x150": [1] * 150,        # lt from global memory
}


@pytest.mark.parametrize("M", [2, 1024])
@pytest.mark.parametrize("B", [64, 100])
@pytest.mark.parametrize("name", list(PACKINGS))
def test_stream_equals_the_one_shot_decode_and_the_restatement(name, B, M, block):
    Ns = PACKINGS[name]
    K = len(Ns)
    models = _init_models(Ns, M)
    lms = [V.log_model(*m) for m in models]
    rng = np.random.default_rng(K + B + M)
    lt = cases.random_prices(rng, K, 0.2)
    block(B)
    for T in (0, 1, B - 1, B, B + 1, 300):
        sym = rng.integers(0, M, T).astype(np.uint16)
        want = hmm.segment_trans(models, sym, [0, T], lt)
        assert want["status"][0] == 0
        rest, _ = ST.decode(lms, sym, lt, B, [T])
        final_after = {p: rest.final_after(p) for p in range(0, T + 1, B)}
        for pname, feeds in _patterns(T, B).items():
            seen = []

            def on_feed(s, at, parts):
                n = sum(len(x["cls"]) for x in parts)
                assert s.final_frames == final_after[at // B * B] == n, (name, B, M, T, pname, at)
                seen.append(n)

            got = _stream(models, sym, lt, feeds, on_feed)
            _assert_one_shot(got, want, (name, B, M, T, pname))  # (the frames taken after every feed are this one's prefix: they are all of got)
            _assert_restatement(got, rest, (name, B, M, T, pname))
            assert seen == got["finals"] and got["stats"]["peak_pending"] <= T
            assert T == 0 or got["kernel_ms"] > 0.0


def _special_prices(kind, K, rng):
    if kind == "all_forbidden":
        return np.full((K, K), NINF)
    if kind == "all_zero":
        return np.zeros((K, K))
    lt = cases.random_prices(rng, K, 0.0)
    if kind == "forbidden_row":
        lt[1, :] = NINF
    else:
        lt[:, 1] = NINF
    return lt


@pytest.mark.parametrize("kind", ["all_forbidden", "all_zero", "forbidden_row", "forbidden_column"])
@pytest.mark.parametrize("name", ["5x3", "5x13"])
def test_prices_that_forbid_everything_nothing_a_row_or_a_column(name, kind, block):
    Ns, M, T, B = PACKINGS[name], 8, 300, 64
    K = len(Ns)
    models = _init_models(Ns, M)
    lms = [V.log_model(*m) for m in models]
    rng = np.random.default_rng(K)
    lt = _special_prices(kind, K, rng)
    sym = rng.integers(0, M, T).astype(np.uint16)
    want = hmm.segment_trans(models, sym, [0, T], lt)
    assert want["status"][0] == 0
    rest, _ = ST.decode(lms, sym, lt, B, [T])
    for pname, feeds in _patterns(T, B).items():
        got = _stream(models, sym, lt, feeds)
        _assert_one_shot(got, want, (name, kind, pname))
        _assert_restatement(got, rest, (name, kind, pname))
        at = 0
        for n, fin in zip(feeds, got["finals"]):
            at += n
            assert fin == rest.final_after(at // B * B), (pname, at)
        if kind == "all_forbidden":  # (paths of different classes never meet)
            assert got["finals"] == [0] * len(feeds)


@pytest.mark.parametrize("case", [c[0] for c in cases.uniform_cases()])
def test_one_price_everywhere_is_the_one_price_session(case, block):
    """path, ln P* and status of hmm.SegmentStream on the same feeds (the CPU test asserts that the two one-shot
    restatements agree on the path for these inputs)"""
    _name, models, streams = next(c for c in cases.uniform_cases() if c[0] == case)
    K = len(models)
    lt = np.full((K, K), cases.UNIFORM_PRICE)
    for seq in streams:
        for feeds in _patterns(len(seq), 64).values():
            a = _stream(models, seq, lt, feeds)
            b = _stream(models, seq, cases.UNIFORM_PRICE, feeds, cls=hmm.SegmentStream)
            for k in ("cls", "state", "entered"):
                assert _same(a[k], b[k]), (case, len(seq), k)
            assert _bits(np.float64(a["log_prob"])) == _bits(np.float64(b["log_prob"])) and a["status"] == b["status"] == 0


# ---- the ring ----------------------------------------------------------------------------------------------------------------------
def test_a_ring_of_three_blocks_wraps_and_a_feed_makes_room_within_itself(block):
    B = 64
    models = planted_models()
    sym = planted_stream(models, np.random.default_rng(3))
    T = len(sym)
    lt = planted_prices()
    lms = [V.log_model(*m) for m in models]
    want = hmm.segment_trans(models, sym, [0, T], lt)
    block(B, 3 * B * (2 * 12 + 12 * 3))
    for feeds in ([T], [50] * (T // 50) + [T % 50], [1] * T):
        rest, finals = ST.decode(lms, sym, lt, B, feeds, cap=3 * B)
        got = _stream(models, sym, lt, feeds)
        _assert_one_shot(got, want, feeds[0])
        assert got["finals"] == finals and got["stats"]["peak_pending"] == rest.peak_pending <= 3 * B
    assert finals[-1] == rest.final_after(T // B * B)
    # the mirror's segments, completed call by call, are the segments of the whole
    assert got["segments"] == want["segments"][0] and len(got["segments"]) >= 5
    got = _stream(models, sym, lt, [50] * (T // 50) + [T % 50])
    assert got["segments"] == hmm.segments_of_trans(want["cls"], want["entered"], want["exit_score"], want["log_prob"][0], lt)


def test_the_ring_full_error_where_nothing_can_be_decided_and_a_clean_close(block):
    B, M = 64, 8
    models = _init_models([3, 4], M, seed=8)
    lt = np.full((2, 2), NINF)
    row = 2 * 7 + 12 * 2
    block(B, 3 * B * row)
    sym = np.random.default_rng(2).integers(0, M, 4 * B).astype(np.uint16)
    with hmm.SegmentTransStream(models, lt) as s:
        for i in range(3):
            out = s.feed(sym[i * B:(i + 1) * B])
            assert s.final_frames == 0 and len(out["cls"]) == 0
        with pytest.raises(e.Ecoz2Error) as ei:
            s.feed(sym[3 * B:])
        msg = str(ei.value)
        assert ENV_PENDING in msg and "192 frames are pending" in msg and "every price is -inf" in msg and "do not connect the classes" in msg
        assert "0 of the feed's 64 symbols" in msg
        out = s.close()
        want = hmm.segment_trans(models, sym[:3 * B], [0, 3 * B], lt)
        for k in KEYS:
            assert _same(out[k], want[k]), k
        assert out["first"] == 0 and s.final_frames == 3 * B and s.status == 0
        assert _bits(np.float64(s.log_prob)) == _bits(want["log_prob"])[0]
        st = s.stats()
        assert st["peak_pending"] == 3 * B
        # the device bytes are set by the budget: the ring of 3 B + B - 1 rows, and little else
        assert (4 * B - 1) * row < st["device_bytes"] < (4 * B - 1) * row + (1 << 16)
        with pytest.raises(e.Ecoz2Error) as ei:
            s.feed(sym[:4])
        assert "e2vq_hmm_segment_stream_feed: the session is closed" in str(ei.value)


# ---- status --------------------------------------------------------------------------------------------------------------------------
def _both(models, lms, sym, lt, B, feeds):
    """the same feeds to the session and to the restatement's Stream, a refused feed ends the feeding -> (got, rest)"""
    rest = ST.Stream(lms, lt, B)
    parts, at = [], 0
    with hmm.SegmentTransStream(models, lt) as s:
        for n in feeds:
            piece = sym[at:at + n]
            at += n
            bad = None
            try:
                rest.feed(piece)
            except ST.BadSymbol as ex:
                bad = ex.frame
            if bad is None:
                parts.append(s.feed(piece))
            else:
                with pytest.raises(e.Ecoz2Error) as ei:
                    s.feed(piece)
                assert f"the symbol at frame {bad} is outside the models' alphabet" in str(ei.value)
            assert s.final_frames == rest.F
            if bad is not None:
                break
        rest.close()
        parts.append(s.close())
        got = {k: np.concatenate([p[k] for p in parts]) for k in KEYS}
        got.update(log_prob=s.log_prob, status=s.status, total=s.final_frames)
    return got, rest


STATUS_FEEDS = {"whole": [130], "blocks": [100, 30], "63_64_3": [63, 64, 3]}


@pytest.mark.parametrize("pname", list(STATUS_FEEDS))
@pytest.mark.parametrize("at", [0, 63, 64, 99, 100, 129])
def test_a_symbol_outside_the_alphabet(at, pname, block):
    B, M, T = 100, 8, 130
    models = _init_models([5] * 13, M)
    lms = [V.log_model(*m) for m in models]
    rng = np.random.default_rng(6)
    lt = cases.random_prices(rng, 13, 0.2)
    sym = rng.integers(0, M, T).astype(np.uint16)
    sym[at] = M
    block(B)
    got, rest = _both(models, lms, sym, lt, B, STATUS_FEEDS[pname])
    assert (got["status"], got["log_prob"], rest.status, rest.log_prob) == (2, NINF, 2, NINF)
    assert got["total"] == rest.F == len(got["cls"])
    _assert_restatement(got, rest, (at, pname))
    assert got["cls"][at:].tolist() == [0xFFFF] * (got["total"] - at)  # (no frame from the bad one on is ever final)


@pytest.mark.parametrize("at", [63, 64, 99, 100])
def test_a_symbol_no_class_can_emit(at, block):
    """every state dies at `at`: nothing more becomes final before close, which reports status 1 and ln P* = -inf (the frames
    are held against the restatement's session on the same feeds, not against the closed decode)"""
    B, M, T = 100, 8, 130
    models = _init_models([3, 4], M, seed=8)
    for pi, A, Bm in models:
        Bm[:, 7] = 0.0
        Bm /= Bm.sum(axis=1, keepdims=True)
    lms = [V.log_model(*m) for m in models]
    lt = np.array([[-1.0, -2.5], [-0.5, NINF]])
    sym = np.random.default_rng(2).integers(0, 7, T).astype(np.uint16)
    sym[at] = 7
    block(B)
    assert hmm.segment_trans(models, sym, [0, T], lt)["status"][0] == 1
    for pname, feeds in STATUS_FEEDS.items():
        got, rest = _both(models, lms, sym, lt, B, feeds)
        assert (got["status"], got["log_prob"], got["total"]) == (1, NINF, T) and rest.status == 1
        assert got["cls"].tolist() == rest.cls and got["state"].tolist() == rest.state and got["entered"].tolist() == rest.entered, pname
        assert _same(got["exit_score"], np.array(rest.exit_score)), pname


def test_more_than_16_wave_slots_are_refused(block):
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.SegmentTransStream(_init_models([64] * 17, 4), np.zeros((17, 17)))
    assert "the classes take 17 wave-slots of 64 lanes (at most 16" in str(ei.value)


# ---- symbols in a device tensor ----------------------------------------------------------------------------------------------------
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
with hmm.SegmentTransStream(models, d["lt"]) as s:
    for a in range(0, len(dev), 90):
        parts.append(s.feed(dev[a:a + 90]))
    parts.append(s.close())
    np.savez(sys.argv[3], log_prob=s.log_prob, status=s.status, **{k: np.concatenate([p[k] for p in parts]) for k in ("cls", "state", "entered", "exit_score")})
print("ok")
"""


def test_symbols_in_a_device_tensor(tmp_path, block):
    models = _init_models([5, 5, 5], 64, seed=3)
    sym = np.random.default_rng(9).integers(0, 64, 300).astype(np.uint16)
    lt = cases.random_prices(np.random.default_rng(1), 3, 0.2)
    ref = hmm.segment_trans(models, sym, [0, 300], lt)
    np.savez(tmp_path / "in.npz", pi=np.stack([m[0] for m in models]), A=np.stack([m[1] for m in models]),
             B=np.stack([m[2] for m in models]), sym=sym, lt=lt)
    r = subprocess.run([sys.executable, "-c", _TORCH_SCRIPT, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
    got = np.load(tmp_path / "out.npz")
    for k in KEYS:
        assert _same(got[k], ref[k]), k
    assert _bits(got["log_prob"]) == _bits(ref["log_prob"])[0] and got["status"] == 0


# ---- files and CLI -----------------------------------------------------------------------------------------------------------------
def test_grammar_continuous_files_equal_the_concatenated_recording(tmp_path):
    env = dict(os.environ)
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_GPUS", "ECOZ2_HMM_SEGMENT_BODY", "ECOZ2_HMM_SEGMENT_CHUNK_BYTES", ENV_PENDING):
        env.pop(k, None)
    env[ENV_BLOCK] = "64"
    P, M, ls = 4, 16, -5.0
    models = planted_models()
    names = ["a", "b", "c"]
    for c, m in zip(names, models):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)
    hmm.write_class_transitions(tmp_path / "t.csv", names, planted_prices() + 5.0)  # (the CLI adds the switch penalty)
    hmm.write_class_transitions(tmp_path / "zeros.csv", names, np.zeros((3, 3)))
    sym = planted_stream(models, np.random.default_rng(3))
    cuts = [0, 170, 171, len(sym)]  # (a piece of one frame among them)
    (tmp_path / "seq").mkdir()
    for i in range(3):
        e.formats.write_seq(str(tmp_path / "seq" / f"p{i}.seq"), "_", M, sym[cuts[i]:cuts[i + 1]])
    e.formats.write_seq(str(tmp_path / "cat.seq"), "_", M, sym)
    rng = np.random.default_rng(5)
    e.formats.write_cbook(str(tmp_path / "cb.cbook"), "_", np.hstack([np.zeros((M, 1)), rng.uniform(-0.8, 0.8, (M, P))]))
    prd = np.hstack([np.ones((400, 1)), rng.uniform(-0.5, 0.5, (400, P))])
    pcuts = [0, 130, 300, 400]
    (tmp_path / "prd").mkdir()
    for i in range(3):
        e.formats.write_prd(str(tmp_path / "prd" / f"p{i}.prd"), "_", prd[pcuts[i]:pcuts[i + 1]])
    e.formats.write_prd(str(tmp_path / "cat.prd"), "_", prd)

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

    for kind, flag, ext, extra in (("seq", "--sequences", ".seq", []), ("prd", "--predictors", ".prd", ["--codebook", "cb.cbook"])):
        whole = run(*extra, "-c", f"one_{kind}", "--class-transitions", "t.csv", flag, f"cat{ext}")
        parts = run(*extra, "-c", f"cont_{kind}", "--class-transitions", "t.csv", "--grammar-continuous", "rec", flag,
                    *[f"{kind}/p{i}{ext}" for i in range(3)])
        want = (tmp_path / f"one_{kind}" / "cat.csv").read_bytes()
        assert (tmp_path / f"cont_{kind}" / "rec.csv").read_bytes() == want and want.count(b"\n") >= 3  # (at least two segments)
        assert sorted(os.listdir(tmp_path / f"cont_{kind}")) == ["rec.csv"]
        b1, b2 = block_of(whole, f"cat{ext}"), block_of(parts, "rec")
        assert b2[0] == "rec" + b1[0][len(f"cat{ext}"):] and b2[1:] == b1[1:]
    # the Python mirror of the file form; -c <file.csv> names the file itself
    want = (tmp_path / "one_seq" / "cat.csv").read_bytes()
    hmm_files = [str(tmp_path / "hmms" / f"{c}.hmm") for c in names]
    pieces = [str(tmp_path / "seq" / f"p{i}.seq") for i in range(3)]
    os.environ[ENV_BLOCK] = "64"
    try:
        hmm.segment_files(hmm_files, pieces, ls, P=P, csv=tmp_path / "py" / "x.csv", class_transitions=tmp_path / "t.csv",
                          grammar_continuous="rec")
    finally:
        del os.environ[ENV_BLOCK]
    assert (tmp_path / "py" / "x.csv").read_bytes() == want
    # a file of zeros: every succession costs the switch penalty, and the CSV is that of --continuous byte for byte
    run("-c", "zeros", "--class-transitions", "zeros.csv", "--grammar-continuous", "rec", "--sequences", *[f"seq/p{i}.seq" for i in range(3)])
    run("-c", "one_price", "--continuous", "rec", "--sequences", *[f"seq/p{i}.seq" for i in range(3)])
    assert (tmp_path / "zeros" / "rec.csv").read_bytes() == (tmp_path / "one_price" / "rec.csv").read_bytes() != want
