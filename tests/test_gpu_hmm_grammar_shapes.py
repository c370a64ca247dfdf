"""`hmm transitions --em`, `hmm learn --loop` and `hmm segment --grammar-continuous` on the GPU where
their own files do not take them, on the inputs of tests/hmm_class_loop_cases.py, every comparison bit for bit (limbs as
int64, doubles as their 64 bits, status; no tolerance): a named row for each instantiation of k_hmm_trans_estep<A_LDS, W_LDS>,
k_hmm_loop_estep<A_LDS, W_LDS, GRAM> and k_hmm_segment_trans_stream<A_LDS, LT_LDS>, for each place of the AN and C tables next
to each place of A and w, and for the launch above 64 KB of dynamic LDS wherever one can be -- one of them at the LDS cap
exactly --, against the numpy restatements and against the sibling passes on the GPU; the session at rows whose paths visit
many classes, so that the coalescence delivers frames mid-stream, in three feed patterns; a symbol outside the alphabet and a
symbol no state emits at the edges of the 64-symbol hand-out and at the last frame under the two trainers, behind a batch of
clean streams and behind a chunk that is not the first; the seeded random sets; one iteration of the training through two
wide layouts.  The layout and the bytes of every launch are asserted through route() in test_hmm_class_loop_cases_cpu.py."""
import time

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_class_loop_cases as cases
from . import hmm_loop_em_restatement as RL
from . import hmm_transitions_em_restatement as RE
from . import hmm_viterbi_restatement as V
from .test_gpu_hmm_loop_em import _assert_equal as _assert_loop
from .test_gpu_hmm_loop_em import _models_equal
from .test_gpu_hmm_segment_trans_stream import _assert_one_shot, _assert_restatement, _both, _same, _stream
from .test_gpu_hmm_transitions_em import _assert_equal as _assert_trans
from .test_gpu_hmm_transitions_em import _bits

pytestmark = pytest.mark.gpu

NINF = float("-inf")
CHUNK = "ECOZ2_HMM_POSTERIOR_CHUNK_BYTES"
TRANS_C, LOOP_AN, LOOP_C = "ECOZ2_HMM_TRANS_EM_C", "ECOZ2_HMM_LOOP_EM_AN", "ECOZ2_HMM_LOOP_EM_C"
ENV_BLOCK, ENV_PENDING = "ECOZ2_HMM_SEGMENT_STREAM_BLOCK", "ECOZ2_HMM_SEGMENT_STREAM_PENDING_BYTES"


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in (CHUNK, TRANS_C, LOOP_AN, LOOP_C, "ECOZ2_HMM_SEGMENT_BODY", "ECOZ2_HMM_SEGMENT_CHUNK_BYTES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(ENV_BLOCK, str(cases.SESSION_B))
    monkeypatch.setenv(ENV_PENDING, str(16 << 20))  # (the default ring of 256 MiB is not needed here)


def _ns(models):
    return [len(m[0]) for m in models]


def _where(r, keys):
    return "".join("-" if r[k] is None else "FT"[r[k]] for k in keys) + " %d B" % r["lds"]


# ---- 1. transitions_estep at every row -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.GRAMMAR_SHAPES))
def test_transitions_estep_equals_the_restatement_at_every_row(name, monkeypatch):
    models, stream, lt = cases.grammar_shape(name)
    T, K = len(stream), len(models)
    want = cases.trans_estep_reference(name)
    t0 = time.perf_counter()
    got = hmm.transitions_estep(models, stream, [0, T], lt)
    print(name, "c a w:", _where(cases.route("trans_estep", _ns(models)), ("c_lds", "a_lds", "w_lds")), "call %.3f s, kernel %.1f ms"
          % (time.perf_counter() - t0, hmm.transitions_estep_last_kernel_ms()))
    _assert_trans(got, want, name)
    assert got["status"].tolist() == [0] and got["acc"].shape == (2 * K * K + 2,) and got["acc"][-2:].tolist() == [1, 0]
    assert got["acc"][:-2].any() and T == cases.GRAMMAR_SHAPES[name][2]
    _assert_trans(got, hmm.segment_trans_posteriors(models, stream, [0, T], lt), name, keys=("log_prob", "status"))
    if name in ("64x3", "1x80"):  # the count table in global memory next to A and w in LDS
        r = cases.route("trans_estep", _ns(models), c=False)
        assert (r["c_lds"], r["a_lds"], r["w_lds"]) == (False, True, True) and cases.route("trans_estep", _ns(models))["c_lds"]
        monkeypatch.setenv(TRANS_C, "global")
        _assert_trans(hmm.transitions_estep(models, stream, [0, T], lt), want, (name, "global"))
    if name == "40_1x24_x6":  # 150 classes: the table does not fit, and the host says so before any launch
        assert cases.route("trans_estep", _ns(models), c=True)["lds"] > cases.SEG_LDS_BYTES
        monkeypatch.setenv(TRANS_C, "lds")
        with pytest.raises(e.Ecoz2Error) as ei:
            hmm.transitions_estep(models, stream, [0, T], lt)
        assert "bytes of LDS" in str(ei.value)


# ---- 2. loop_estep at every row --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.GRAMMAR_SHAPES))
def test_loop_estep_equals_the_restatement_at_every_row(name, monkeypatch):
    models, stream, lt = cases.grammar_shape(name)
    T, K = len(stream), len(models)
    Ns = _ns(models)
    want = cases.loop_estep_reference(name)
    t0 = time.perf_counter()
    got = hmm.loop_estep(models, stream, [0, T], lt, acc_trans=True)
    keys = ("an_lds", "c_lds", "a_lds", "w_lds")
    print(name, "an c a w:", _where(cases.route("loop_estep", Ns), keys), "call %.3f s, kernel %.1f ms; without the table:"
          % (time.perf_counter() - t0, hmm.loop_estep_last_kernel_ms()), _where(cases.route("loop_estep", Ns, gram=False), keys))
    _assert_loop(got, want, name)
    assert got["status"].tolist() == [0] and got["acc_trans"][-2:].tolist() == [1, 0] and got["acc_trans"][:-2].any()
    for a, (pi, _A, B) in zip(got["acc"], models):
        lay = RL.layout(len(pi), B.shape[1])
        assert (a[lay["used"]], a[lay["skipped"]]) == (1, 0) and a[:lay["used"]].any()
    # without the grammar table (GRAM = false, and at some rows another layout): the same state limbs
    plain = hmm.loop_estep(models, stream, [0, T], lt)
    assert "acc_trans" not in plain
    _assert_loop(plain, got, (name, "plain"), keys=("acc", "log_prob", "status"))
    # the grammar limbs: the sibling pass on the GPU
    _assert_loop(got, dict(acc_trans=hmm.transitions_estep(models, stream, [0, T], lt)["acc"]), name, keys=("acc_trans",))
    if name == "64x2":  # AN in LDS next to A in global memory: each forced route changes the layout, none a limb
        pick = lambda r: tuple(r[k] for k in keys)
        free = cases.route("loop_estep", Ns)
        for var, kw in ((LOOP_AN, dict(an=False)), (LOOP_C, dict(c=False))):
            forced = cases.route("loop_estep", Ns, **kw)
            assert pick(forced) != pick(free) == (True, True, False, True), (var, forced)
            monkeypatch.setenv(var, "global")
            _assert_loop(hmm.loop_estep(models, stream, [0, T], lt, acc_trans=True), want, (name, var))
            monkeypatch.delenv(var)
        assert cases.route("loop_estep", Ns, an=False)["a_lds"] and not cases.route("loop_estep", Ns, c=False)["c_lds"]


# ---- 3. the session at every row -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.GRAMMAR_SHAPES))
def test_the_grammar_session_equals_the_one_shot_decode_and_the_restatement_at_every_row(name):
    models, stream, lt = cases.grammar_shape(name)
    T, B = len(stream), cases.SESSION_B
    rest, final_after = cases.trans_stream_reference(name)
    want = hmm.segment_trans(models, stream, [0, T], lt)
    assert want["status"].tolist() == [0]
    print(name, "a lt:", _where(cases.route("trans_stream", _ns(models)), ("a_lds", "lt_lds")), "final after each block:",
          [final_after[p] for p in range(B, T + 1, B)])
    # (K = 772 and K = 1024: whole blocks are enough; the other patterns change the host's buffering alone)
    patterns = ("whole_blocks",) if name in ("1x1024", "64x4_1x768") else ("whole", "whole_blocks", "63_64_65")
    for pattern in patterns:
        feeds = cases.session_feeds(T, pattern)
        seen = []

        def on_feed(s, at, parts):
            n = sum(len(x["cls"]) for x in parts)
            assert s.final_frames == final_after[at // B * B] == n, (name, pattern, at)
            seen.append(n)

        got = _stream(models, stream, lt, feeds, on_feed)
        _assert_one_shot(got, want, (name, pattern))
        _assert_restatement(got, rest, (name, pattern))
        assert seen == got["finals"] and len(seen) == len(feeds)
        if pattern == "whole_blocks":  # frames were delivered before close (which ones: the CPU file's condition)
            assert 2 * sum(f > 0 for f in seen[:T // B]) >= T // B


# ---- 4. events at the edges of the 64-symbol hand-out ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.GRAMMAR_EVENT_SETS)
def test_the_trainers_meet_a_bad_and_a_dead_symbol_at_the_edges_of_the_hand_out(name, monkeypatch):
    streams, kinds = cases.event_batch()
    sym, offs = hmm._pack(streams)
    models = cases.event_models(name)
    K, T, S = len(models), cases.EVENT_T, len(streams)
    lt = cases.event_prices(K)
    status = [cases.event_status(k, "trans_posteriors") for k in kinds]  # the first event in frame order decides
    assert status == [0] + [2] * 6 + [1] * 6 + [1, 2] * 3
    want_t, want_l = cases.grammar_event_reference(name)
    lays = [RL.layout(len(pi), B.shape[1]) for pi, _A, B in models]
    clean_sym = np.tile(sym[:T], S)
    for budget in (None, "1"):  # "1": one stream per launch, so that a0 of an event stream is not 0
        if budget is not None:
            monkeypatch.setenv(CHUNK, budget)
        note = (name, budget)
        # ---- hmm transitions --em.  A batch of clean streams goes first: the buffers the next call is handed hold data.
        alone = hmm.transitions_estep(models, sym[:T], [0, T], lt)
        _assert_trans(alone, want_t, note)
        clean = hmm.transitions_estep(models, clean_sym, offs, lt)
        assert clean["status"].tolist() == [0] * S and clean["acc"][-2:].tolist() == [S, 0], note
        assert np.array_equal(clean["acc"][:-2], S * alone["acc"][:-2]) and alone["acc"][:-2].any(), note
        got = hmm.transitions_estep(models, sym, offs, lt)
        assert got["status"].tolist() == status, note
        assert _same(got["log_prob"][:1], alone["log_prob"]) and (got["log_prob"][1:] == NINF).all(), note
        assert np.array_equal(got["acc"][:-2], alone["acc"][:-2]) and got["acc"][-2:].tolist() == [1, S - 1], note
        # ---- hmm learn --loop, with the grammar table
        alone = hmm.loop_estep(models, sym[:T], [0, T], lt, acc_trans=True)
        _assert_loop(alone, want_l, note)
        clean = hmm.loop_estep(models, clean_sym, offs, lt, acc_trans=True)
        assert clean["status"].tolist() == [0] * S and clean["acc_trans"][-2:].tolist() == [S, 0], note
        assert np.array_equal(clean["acc_trans"][:-2], S * alone["acc_trans"][:-2]), note
        gotl = hmm.loop_estep(models, sym, offs, lt, acc_trans=True)
        assert gotl["status"].tolist() == status, note
        assert _same(gotl["log_prob"][:1], alone["log_prob"]) and (gotl["log_prob"][1:] == NINF).all(), note
        assert np.array_equal(gotl["acc_trans"], got["acc"]), note
        for k, (a, b, c, lay) in enumerate(zip(gotl["acc"], alone["acc"], clean["acc"], lays)):
            u = lay["used"]
            assert np.array_equal(a[:u], b[:u]) and b[:u].any() and np.array_equal(c[:u], S * b[:u]), (note, k)
            assert a[u:].tolist() == [1, S - 1] and b[u:].tolist() == [1, 0] and c[u:].tolist() == [S, 0], (note, k)
        plain = hmm.loop_estep(models, sym, offs, lt)
        _assert_loop(plain, gotl, note, keys=("acc", "log_prob", "status"))


def test_the_session_is_the_one_shot_decode_at_a_bad_symbol_in_the_last_frame_with_lA_and_lt_global():
    # k_hmm_segment_trans_stream<false, false>; frame 129 waits in the remainder and reaches the kernel only at close
    models = cases.event_models("40_1x24_x14")
    K, T, B = len(models), cases.EVENT_T, cases.SESSION_B
    r = cases.route("trans_stream", _ns(models))
    assert (r["a_lds"], r["lt_lds"]) == (False, False)
    lt = cases.event_prices(K)
    clean = cases.event_batch()[0][0]
    sym = cases.with_symbols(clean, {T - 1: cases.EVENT_M})
    lms = [V.log_model(*m) for m in models]
    want = hmm.segment_trans(models, sym, [0, T], lt)
    whole = hmm.segment_trans(models, clean, [0, T], lt)
    assert want["status"].tolist() == [2] and whole["status"].tolist() == [0]
    for feeds in ([T], [B, T - B], [63, 64, T - 127]):
        got, rest = _both(models, lms, sym, lt, B, feeds)
        assert (got["status"], got["log_prob"], rest.status, rest.log_prob) == (2, NINF, 2, NINF), feeds
        assert got["status"] == want["status"][0] and _same(np.float64(got["log_prob"]), want["log_prob"][0])
        assert got["total"] == rest.F == T == len(got["cls"])
        _assert_restatement(got, rest, feeds)
        # what was delivered before close is the clean stream's path; the rest is the one-shot decode's fill
        n = int(np.argmax(got["cls"] == 0xFFFF))
        assert n == rest.final_after(T // B * B) and (got["cls"][n:] == 0xFFFF).all()
        for k in ("cls", "state", "entered", "exit_score"):
            assert _same(got[k][:n], whole[k][:n]), (k, feeds)
            assert _same(got[k][max(n, 1):], want[k][max(n, 1):]), (k, feeds)


# ---- 5. the random sets ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_resident():
    return cases.random_sets(cases.RANDOM_SEED, resident_only=True)


# what the draw gives each launcher above 64 KB (asserted, so that a later change of the draw cannot lose it): kernel -> set ->
# the places its route() names, in the order of the keys below
RANDOM_KEYS = {"trans_estep": ("c_lds", "a_lds", "w_lds"), "loop_estep": ("an_lds", "c_lds", "a_lds", "w_lds"),
               "trans_stream": ("a_lds", "lt_lds")}
RANDOM_ABOVE_64_KB = {
    "trans_estep": {1: (True, True, True), 8: (True, True, True), 11: (True, True, True)},
    "loop_estep": {1: (False, True, True, True), 3: (True, True, True, True), 8: (False, True, True, True), 11: (False, True, True, True)},
    "trans_stream": {0: (True, True), 1: (True, True), 8: (True, True), 11: (True, True)},
}


@pytest.mark.parametrize("i", range(12))  # (a case per set: the restatements of a set take up to three seconds)
def test_the_trainers_and_the_session_on_the_random_sets(i, random_resident):
    row = random_resident[i]
    Ns, K = row["Ns"], len(row["Ns"])
    for kernel, keys in RANDOM_KEYS.items():
        r = cases.route(kernel, Ns)
        assert (r["lds"] > cases.LDS_OPT_IN) == (i in RANDOM_ABOVE_64_KB[kernel]), (kernel, r)
        if i in RANDOM_ABOVE_64_KB[kernel]:
            assert tuple(r[k] for k in keys) == RANDOM_ABOVE_64_KB[kernel][i], (kernel, r)
    sym, offs = hmm._pack(row["streams"])  # the six streams in one call
    lt = cases.forbidding_prices(i, K)
    got = hmm.transitions_estep(row["models"], sym, offs, lt)
    _assert_trans(got, RE.estep(row["models"], sym, offs, lt), (i, Ns))
    gotl = hmm.loop_estep(row["models"], sym, offs, lt, acc_trans=True)
    _assert_loop(gotl, RL.estep(row["models"], sym, offs, lt, acc_trans=True), (i, Ns))
    assert np.array_equal(gotl["acc_trans"], got["acc"])
    # the session on the longest stream
    seq = max(row["streams"], key=len)
    T = len(seq)
    want = hmm.segment_trans(row["models"], seq, [0, T], lt)
    assert want["status"].tolist() == [0] and T > 64
    _assert_one_shot(_stream(row["models"], seq, lt, cases.session_feeds(T, "63_64_65")), want, (i, Ns))


# ---- 6. one iteration of the training through a wide layout ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["64x2", "40_1x24_x14"])  # AN in LDS next to A global; everything global, 350 classes
def test_one_iteration_of_the_training_equals_the_restatements_loop(name):
    models, stream, lt = cases.grammar_shape(name)
    T = len(stream)
    kw = dict(ln_p=lt, ln_switch=0.0, train_transitions=True, alpha=0.5, max_iterations=1)
    got, got_p, hist = hmm.train_loop(models, stream, [0, T], **kw)
    want, want_p, whist = RL.train(models, stream, [0, T], **kw)
    assert len(hist) == len(whist) == 1 and np.array_equal(_bits(hist), _bits(np.array(whist)))
    _models_equal(got, want, name)
    assert np.array_equal(_bits(got_p), _bits(want_p))
    assert np.array_equal(got_p == NINF, lt == NINF) and not np.array_equal(got_p, lt)  # a forbidden succession stays forbidden
    assert any(not np.array_equal(g[1], m[1]) for g, m in zip(got, models))  # (the M-step ran: A has moved)
