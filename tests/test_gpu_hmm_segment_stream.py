"""`hmm segment --continuous` on the GPU: the session against e2vq_hmm_segment on the concatenation, bit
for bit, for every packing, body, block length and feed pattern; the frames it delivers after every feed against the
restatement's finality rule; the bound on the pending frames; the status rules; the file form and the CLI against `hmm
segment --sequences` on the concatenated file; the Python mirror's segments."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_segment_restatement as R
from . import hmm_segment_stream_restatement as S
from . import hmm_viterbi_restatement as V
from .test_hmm_segment_stream_cpu import planted_models, planted_stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
NINF = float("-inf")
ENV_BLOCK = "ECOZ2_HMM_SEGMENT_STREAM_BLOCK"
ENV_PENDING = "ECOZ2_HMM_SEGMENT_STREAM_PENDING_BYTES"
KEYS = ("cls", "state", "entered", "gbest")


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


def _stream(models, sym, ls, feeds, on_feed=None):
    """the session fed sym in pieces of the lengths `feeds`, closed -> dict of all frames, log_prob, status, finals"""
    parts, finals, at = [], [], 0
    with hmm.SegmentStream(models, ls) as s:
        for n in feeds:
            parts.append(s.feed(sym[at:at + n]))
            at += n
            finals.append(s.final_frames)
            if on_feed:
                on_feed(s, at, parts)
        assert at == len(sym)
        parts.append(s.close())
        out = {k: np.concatenate([p[k] for p in parts]) for k in KEYS}
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


def _patterns(T, rng):
    rand = []
    while sum(rand) < T:
        rand.append(int(min(rng.choice([0, 0, 1, 5, 17, 64, 90, 130]), T - sum(rand))))
    cyc, i = [], 0
    while sum(cyc) < T:
        cyc.append(min((63, 64, 65)[i % 3], T - sum(cyc)))
        i += 1
    return {"whole": [T], "single": [1] * T, "63_64_65": cyc, "random": rand + [0]}


# ---- equality with e2vq_hmm_segment ----------------------------------------------------------------------------------------
PACKINGS = {
    "5x13": ([5] * 13, None),                # two packed slots
    "3_64_7_7_33": ([3, 64, 7, 7, 33], None),  # packed next to one-class slots
    "64x16": ([64] * 16, None),              # 16 slots, resident, lA from global memory
    "64x17": ([64] * 17, None),              # the first looped shape
    "33x20": ([33] * 20, None),              # looped, two slots to some waves
    "5x13_looped": ([5] * 13, "looped"),     # ECOZ2_HMM_SEGMENT_BODY=looped, honoured by the session
}


@pytest.mark.parametrize("B", [64, 100])
@pytest.mark.parametrize("name", list(PACKINGS))
def test_stream_equals_the_one_shot_decode(name, B, block, monkeypatch):
    Ns, body = PACKINGS[name]
    M, T, ls = 8, 400, -3.0
    models = _init_models(Ns, M)
    rng = np.random.default_rng(len(Ns) + B)
    sym = rng.integers(0, M, T).astype(np.uint16)
    want = hmm.segment(models, sym, [0, T], ls)
    assert want["status"][0] == 0
    block(B)
    if body:
        monkeypatch.setenv("ECOZ2_HMM_SEGMENT_BODY", body)
    counts = {}
    for pname, feeds in _patterns(T, rng).items():
        got = _stream(models, sym, ls, feeds)
        _assert_one_shot(got, want, (name, B, pname))
        # the frames final after p processed frames do not depend on how they were fed
        at = 0
        for n, fin in zip(feeds, got["finals"]):
            at += n
            assert counts.setdefault(at // B * B, fin) == fin, (pname, at)
        assert got["kernel_ms"] > 0.0 and got["stats"]["peak_pending"] <= T
    assert sorted(counts) == list(range(0, T + 1, B))  # (the single symbols stop at every multiple of B)


# ---- online delivery ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["planted", "random_5x13"])
def test_frames_are_delivered_as_the_finality_rule_decides_them(case, block):
    B = 64
    if case == "planted":
        models, ls = planted_models(), -5.0
        sym = planted_stream(models, np.random.default_rng(3))
    else:
        models, ls = _init_models([5] * 13, 16), -3.0
        sym = np.random.default_rng(4).integers(0, 16, 450).astype(np.uint16)
    T = len(sym)
    lms = [V.log_model(*m) for m in models]
    want = hmm.segment(models, sym, [0, T], ls)
    feeds = [50] * (T // 50) + [T % 50]
    rest, _ = S.decode(lms, sym, ls, B, feeds)
    assert rest.join_failures == 0
    seen = []

    def on_feed(s, at, parts):
        p = at // B * B
        assert s.final_frames == rest.final_after(p), (at, p)
        n = sum(len(x["cls"]) for x in parts)
        assert n == s.final_frames  # (everything final has been handed out)
        for k in KEYS:
            assert _same(np.concatenate([x[k] for x in parts]), want[k][:n]), (k, at)
        seen.append((p, s.final_frames))

    got = _stream(models, sym, ls, feeds, on_feed)
    _assert_one_shot(got, want)
    print(case, "(processed, final) after each feed:", seen, "peak pending:", got["stats"]["peak_pending"])
    if case == "planted":  # (the CPU tests assert this of the restatement: at least half from the second block on)
        assert all(2 * f >= p for p, f in seen if p >= 2 * B)
        assert got["stats"]["peak_pending"] == rest.peak_pending


# ---- bounded memory ---------------------------------------------------------------------------------------------------------------
def test_the_pending_frames_are_bounded_and_close_still_decodes(block):
    B, M = 64, 8
    models = _init_models([3, 4], M, seed=8)
    row = 2 * 7 + 4
    block(B, 3 * B * row)
    sym = np.random.default_rng(2).integers(0, M, 4 * B).astype(np.uint16)
    with hmm.SegmentStream(models, NINF) as s:
        for i in range(3):
            out = s.feed(sym[i * B:(i + 1) * B])
            assert s.final_frames == 0 and len(out["cls"]) == 0  # (paths of the two classes never meet)
        with pytest.raises(e.Ecoz2Error) as ei:
            s.feed(sym[3 * B:])
        msg = str(ei.value)
        assert ENV_PENDING in msg and "192 frames are pending" in msg and "ln_switch = -inf" in msg and "0 of the feed's 64 symbols" in msg
        out = s.close()
        want = hmm.segment(models, sym[:3 * B], [0, 3 * B], NINF)
        for k in KEYS:
            assert _same(out[k], want[k]), k
        assert out["first"] == 0 and s.final_frames == 3 * B and s.status == 0
        assert _bits(np.float64(s.log_prob)) == _bits(want["log_prob"])[0]
        assert len(set(out["cls"].tolist())) == 1 and out["entered"].tolist() == [1] + [0] * (3 * B - 1)  # the best single model's path
        assert s.stats()["peak_pending"] == 3 * B


def test_a_small_ring_wraps_and_a_feed_makes_room_within_itself(block):
    """a budget of three blocks on the planted stream: the ring's rows are reused several times over, and a feed of the whole
    stream has to run a coalescence between its blocks to go on"""
    B, ls = 64, -5.0
    models = planted_models()
    sym = planted_stream(models, np.random.default_rng(3))
    T = len(sym)
    lms = [V.log_model(*m) for m in models]
    want = hmm.segment(models, sym, [0, T], ls)
    block(B, 3 * B * (2 * 12 + 4))
    for feeds in ([T], [50] * (T // 50) + [T % 50], [1] * T):
        rest, finals = S.decode(lms, sym, ls, B, feeds, cap=3 * B)
        got = _stream(models, sym, ls, feeds)
        _assert_one_shot(got, want, feeds[0])
        assert got["finals"] == finals and got["stats"]["peak_pending"] == rest.peak_pending <= 3 * B
    assert finals[-1] == rest.final_after(T // B * B)


# ---- status ----------------------------------------------------------------------------------------------------------------------
def test_a_symbol_outside_the_alphabet(block):
    B, M, T, ls = 64, 8, 300, -3.0
    models = _init_models([5] * 13, M)
    lms = [V.log_model(*m) for m in models]
    sym = np.random.default_rng(6).integers(0, M, T).astype(np.uint16)
    sym[2 * B + 10] = M
    rest = S.Stream(lms, ls, B)
    rest.feed(sym[:2 * B])
    F0 = rest.F
    assert 0 < F0 < 2 * B
    with hmm.SegmentStream(models, ls) as s:
        head = s.feed(sym[:2 * B])
        assert s.final_frames == F0 and head["cls"].tolist() == rest.cls and head["entered"].tolist() == rest.entered
        assert _same(head["gbest"], np.array(rest.gbest))
        with pytest.raises(e.Ecoz2Error) as ei:
            s.feed(sym[2 * B:])
        assert f"the symbol at frame {2 * B + 10} is outside the models' alphabet of {M}" in str(ei.value)
        assert s.final_frames == F0
        with pytest.raises(e.Ecoz2Error) as ei:
            s.feed(sym[:4])
        assert "takes no more symbols" in str(ei.value)
        with pytest.raises(e.Ecoz2Error):
            s.flush()
        tail = s.close()
        assert (s.status, s.log_prob, s.final_frames) == (2, NINF, T)
        n = T - F0
        assert tail["first"] == F0 and tail["cls"].tolist() == [0xFFFF] * n and tail["state"].tolist() == [0xFFFF] * n
        assert tail["entered"].tolist() == [0] * n and tail["gbest"].tolist() == [NINF] * n and tail["segments"] == []


def test_a_stream_that_dies_an_empty_one_and_one_shorter_than_a_block(block):
    M, ls = 8, -3.0
    # every state dead: each model cannot emit one of the symbols, and no segment may start
    models = _init_models([3, 4], M, seed=8)
    for k, (pi, A, Bm) in enumerate(models):
        Bm[:, 6 + k] = 0.0
        Bm /= Bm.sum(axis=1, keepdims=True)
    sym = np.random.default_rng(2).integers(0, 6, 200).astype(np.uint16)
    sym[70], sym[150] = 6, 7
    want = hmm.segment(models, sym, [0, 200], NINF)
    assert want["status"][0] == 1
    got = _stream(models, sym, NINF, [64, 64, 72])
    assert got["status"] == 1 and got["log_prob"] == NINF and got["total"] == 200
    # nothing fed
    with hmm.SegmentStream(models, ls) as s:
        out = s.close()
        assert (s.log_prob, s.status, s.final_frames) == (0.0, 0, 0) and len(out["cls"]) == 0 and out["segments"] == []
        with pytest.raises(e.Ecoz2Error) as ei:
            s.feed(sym[:4])
        assert "e2vq_hmm_segment_stream_feed: the session is closed" in str(ei.value)
        with pytest.raises(e.Ecoz2Error) as ei:
            s.close()
        assert "the session is closed" in str(ei.value)
    # shorter than one block: decided at close alone
    models = _init_models([5] * 13, M)
    sym = np.random.default_rng(3).integers(0, M, 40).astype(np.uint16)
    got = _stream(models, sym, ls, [25, 15])
    assert got["finals"] == [0, 0]
    _assert_one_shot(got, hmm.segment(models, sym, [0, 40], ls))
    # a flush in between: the remainder is processed, and the next block starts behind it
    sym = np.random.default_rng(3).integers(0, M, 230).astype(np.uint16)
    want = hmm.segment(models, sym, [0, 230], ls)
    lms = [V.log_model(*m) for m in models]
    rest, _ = S.decode(lms, sym, ls, 64, [230])
    with hmm.SegmentStream(models, ls) as s:
        a = s.feed(sym[:70])
        b = s.flush()
        assert s.final_frames == rest.final_after(70)
        c = s.feed(sym[70:])
        assert s.final_frames == rest.final_after(70 + 128)
        d = s.close()
        for k in KEYS:
            assert _same(np.concatenate([x[k] for x in (a, b, c, d)]), want[k]), k
        assert _bits(np.float64(s.log_prob)) == _bits(want["log_prob"])[0]


# ---- the Python mirror's segments; symbols in a device tensor ------------------------------------------------------------------------
def test_segments_completed_call_by_call_are_segments_of_the_whole(block):
    models = planted_models()
    sym = planted_stream(models, np.random.default_rng(3))
    T, ls = len(sym), -5.0
    want = hmm.segment(models, sym, [0, T], ls)
    got = _stream(models, sym, ls, [50] * (T // 50) + [T % 50])
    assert got["segments"] == want["segments"][0] and len(got["segments"]) == 5


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
with hmm.SegmentStream(models, -3.0) as s:
    for a in range(0, len(dev), 90):
        parts.append(s.feed(dev[a:a + 90]))
    parts.append(s.close())
    np.savez(sys.argv[3], log_prob=s.log_prob, status=s.status, **{k: np.concatenate([p[k] for p in parts]) for k in ("cls", "state", "entered", "gbest")})
print("ok")
"""


def test_symbols_in_a_device_tensor(tmp_path, block):
    models = _init_models([5, 5, 5], 64, seed=3)
    sym = np.random.default_rng(9).integers(0, 64, 400).astype(np.uint16)
    ref = hmm.segment(models, sym, [0, 400], -3.0)
    np.savez(tmp_path / "in.npz", pi=np.stack([m[0] for m in models]), A=np.stack([m[1] for m in models]),
             B=np.stack([m[2] for m in models]), sym=sym)
    r = subprocess.run([sys.executable, "-c", _TORCH_SCRIPT, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
    got = np.load(tmp_path / "out.npz")
    for k in KEYS:
        assert _same(got[k], ref[k]), k
    assert _bits(got["log_prob"]) == _bits(ref["log_prob"])[0] and got["status"] == 0


# ---- files and CLI ---------------------------------------------------------------------------------------------------------------
def test_continuous_files_equal_the_concatenated_recording(tmp_path, capfd):
    env = dict(os.environ)
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_GPUS", "ECOZ2_HMM_SEGMENT_BODY", "ECOZ2_HMM_SEGMENT_CHUNK_BYTES", ENV_PENDING):
        env.pop(k, None)
    env[ENV_BLOCK] = "64"
    P, M, ls = 4, 16, -5.0
    models = planted_models()
    names = ["a", "b", "c"]
    for c, m in zip(names, models):
        hmm.save_model(tmp_path / "hmms" / f"{c}.hmm", c, *m)
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
        whole = run(*extra, "-c", f"one_{kind}", flag, f"cat{ext}")
        parts = run(*extra, "-c", f"cont_{kind}", "--continuous", "rec", flag, *[f"{kind}/p{i}{ext}" for i in range(3)])
        want = (tmp_path / f"one_{kind}" / "cat.csv").read_bytes()
        assert (tmp_path / f"cont_{kind}" / "rec.csv").read_bytes() == want and want.count(b"\n") > 3
        assert sorted(os.listdir(tmp_path / f"cont_{kind}")) == ["rec.csv"]
        b1, b2 = block_of(whole, f"cat{ext}"), block_of(parts, "rec")
        assert b2[0] == "rec" + b1[0][len(f"cat{ext}"):] and b2[1:] == b1[1:]
    # -c <file.csv> names the file itself; the Python mirror of the file form
    run("-c", "direct/x.csv", "--continuous", "rec", "--sequences", *[f"seq/p{i}.seq" for i in range(3)])
    want = (tmp_path / "one_seq" / "cat.csv").read_bytes()
    assert (tmp_path / "direct" / "x.csv").read_bytes() == want
    hmm_files = [str(tmp_path / "hmms" / f"{c}.hmm") for c in names]
    pieces = [str(tmp_path / "seq" / f"p{i}.seq") for i in range(3)]
    os.environ[ENV_BLOCK] = "64"
    try:
        hmm.segment_files(hmm_files, pieces, ls, P=P, csv=tmp_path / "py", continuous="rec")
    finally:
        del os.environ[ENV_BLOCK]
    assert (tmp_path / "py" / "rec.csv").read_bytes() == want
    # without --continuous the same inputs are decoded one by one, as e2vq_hmm_segment_files decodes them
    run("-c", "each_cli", "--sequences", *[f"seq/p{i}.seq" for i in range(3)])
    m, _k1 = hmm._strs(hmm_files)
    f, _k2 = hmm._strs(pieces)
    capfd.readouterr()
    assert e.lib.e2vq_hmm_segment_files(m, 3, None, f, 3, P, 45, 15, ls, str(tmp_path / "each_lib").encode()) == 0
    capfd.readouterr()
    for i in range(3):
        assert (tmp_path / "each_cli" / f"p{i}.csv").read_bytes() == (tmp_path / "each_lib" / f"p{i}.csv").read_bytes()
    assert (tmp_path / "each_cli" / "p0.csv").read_bytes() != want
