"""GPU parity of HMM Viterbi decoding: e2vq_hmm_viterbi (k_hmm_viterbi / k_hmm_viterbi_wg +
k_hmm_backtrack) against the numpy restatement -- path, ln P* and status bit for bit -- and `seq show -P / -Q --hmm`
(e2vq_seq_show_files / ecoz2_seq_show_files) through the CLI and the C-ABI, up to an end-to-end chain from predictors."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ecoz2rs_amd as e
from tests import hmm_viterbi_restatement as R
from tests.test_gpu_hmm import _corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
LENGTHS = (0, 1, 2, 63, 64, 65, 300, 5000)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _assert_equal(got, ref, seqs, what=""):
    assert got["status"].tolist() == ref["status"].tolist(), what
    assert np.array_equal(_bits(got["log_prob"]), _bits(ref["log_prob"])), what
    for s in range(len(seqs)):
        assert got["path"][s].dtype == np.uint16 and np.array_equal(got["path"][s], ref["path"][s]), (what, s)


@pytest.mark.parametrize("N,M,types", [(1, 2, (0, 1, 2, 3)), (2, 64, (0, 1, 2, 3)), (5, 1024, (0, 1, 2, 3)),
                                       (13, 2, (0, 1, 2, 3)), (64, 1024, (0, 1, 2, 3)), (65, 64, (0, 1, 2, 3)),
                                       (141, 1024, (0, 1, 2, 3)), (512, 64, (0, 3))])
def test_viterbi_bit_exact(N, M, types):
    """N <= 64: the wave kernel; above: the workgroup kernel.  All four initial model types (random, uniform = all ties,
    cascades = -inf in pi and A) and the lengths around the 64-symbol fetch of the wave kernel"""
    rng = np.random.default_rng(N * 7 + M)
    seqs = [rng.integers(0, M, n).astype(np.uint16) for n in LENGTHS]
    for typ in types:
        e.hmm.set_random_seed(1000 + N + typ)
        pi, A, B = e.hmm.init_model(N, M, typ)
        got = e.hmm.viterbi(pi, A, B, seqs)
        _assert_equal(got, R.viterbi(pi, A, B, seqs), seqs, (N, M, typ))
        assert got["status"][0] == 0 and got["log_prob"][0] == 0.0 and len(got["path"][0]) == 0  # the empty sequence


def test_viterbi_of_a_trained_model():
    rng = np.random.default_rng(8)
    M = 64
    seqs = [rng.integers(0, M, n).astype(np.uint16) for n in rng.integers(20, 200, 24)]
    e.hmm.set_random_seed(9)
    pi, A, B, hist = e.hmm.train(*e.hmm.init_model(6, M, 3), seqs, max_iterations=4)
    assert len(hist) == 4
    got = e.hmm.viterbi(pi, A, B, seqs)
    _assert_equal(got, R.viterbi(pi, A, B, seqs), seqs)
    assert got["status"].tolist() == [0] * len(seqs)


@pytest.mark.parametrize("N", [4, 70])
def test_viterbi_status_codes(N):
    e.hmm.set_random_seed(5)
    pi, A, B = e.hmm.init_model(N, 8, 3)
    B0 = B.copy()
    B0[:, 5] = 0.0  # symbol 5 cannot be emitted by any state
    seqs = [np.array([1, 5, 2, 3], dtype=np.uint16), np.array([1, 2, 3], dtype=np.uint16), np.array([1, 9, 2], dtype=np.uint16),
            np.array([5], dtype=np.uint16), np.array([8], dtype=np.uint16)]
    got = e.hmm.viterbi(pi, A, B0, seqs)
    assert got["status"].tolist() == [1, 0, 2, 1, 2]
    assert got["log_prob"][[0, 2, 3, 4]].tolist() == [-np.inf] * 4 and np.isfinite(got["log_prob"][1])
    assert got["path"][2].tolist() == [0xFFFF] * 3 and got["path"][4].tolist() == [0xFFFF]
    _assert_equal(got, R.viterbi(pi, A, B0, seqs), seqs)  # status 1 still writes the path, by the same rules


@pytest.mark.parametrize("N", [5, 141])
def test_chunks_and_no_path_give_the_same_results(N, monkeypatch):
    rng = np.random.default_rng(N)
    M = 32
    seqs = [rng.integers(0, M, n).astype(np.uint16) for n in rng.integers(0, 400, 40)]
    e.hmm.set_random_seed(77)
    pi, A, B = e.hmm.init_model(N, M, 0)
    one = e.hmm.viterbi(pi, A, B, seqs)
    _assert_equal(one, R.viterbi(pi, A, B, seqs), seqs)
    for budget in ("1", str(2 * N * 700)):  # one sequence per launch; a few sequences per launch
        monkeypatch.setenv("ECOZ2_HMM_VITERBI_CHUNK_BYTES", budget)
        _assert_equal(e.hmm.viterbi(pi, A, B, seqs), one, seqs, budget)
    monkeypatch.delenv("ECOZ2_HMM_VITERBI_CHUNK_BYTES")
    nopath = e.hmm.viterbi(pi, A, B, seqs, want_path=False)
    assert nopath["path"] is None and nopath["status"].tolist() == one["status"].tolist()
    assert np.array_equal(_bits(nopath["log_prob"]), _bits(one["log_prob"]))


@pytest.mark.parametrize("N,typ", [(5, 0), (5, 3), (64, 0), (100, 2)])
def test_best_path_probability_is_below_the_forward_probability(N, typ):
    rng = np.random.default_rng(N + typ)
    M = 64
    seqs = [rng.integers(0, M, n).astype(np.uint16) for n in (1, 10, 100, 1000)]
    e.hmm.set_random_seed(31 + N)
    pi, A, B = e.hmm.init_model(N, M, typ)
    v = e.hmm.viterbi(pi, A, B, seqs)["log_prob"]
    f = e.hmm.score([(pi, A, B)], seqs)["log_prob"][:, 0]
    for a, b in zip(v, f):
        assert np.isfinite(a) and a <= b + 1e-9 * abs(b)


# ---- seq show -P / -Q ------------------------------------------------------------------------------------------------
def _files(tmp_path, M=16):
    rng = np.random.default_rng(12)
    specs = [("A", M, rng.integers(0, M, 7)), ("B", M, rng.integers(0, M, 31)), ("C", M, rng.integers(0, M, 300)),
             ("D", M, np.zeros(0, dtype=np.int64)), ("E", M, np.array([1, 2, M + 3, 4, M])), ("F", M + 1, rng.integers(0, M, 5))]
    files = []
    for k, (cls, m, sym) in enumerate(specs):
        f = tmp_path / f"{k}_{cls}.seq"
        e.formats.write_seq(str(f), cls, m, np.asarray(sym, dtype=np.uint16))
        files.append(str(f))
    return files


def _cli(*args, cwd=None):
    r = subprocess.run([EXE, "seq", "show", *args], capture_output=True, text=True, timeout=600, cwd=cwd)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_seq_show_prob_and_path_parse_back(tmp_path):
    M = 16
    files = _files(tmp_path, M)
    e.hmm.set_random_seed(4)
    pi, A, B = e.hmm.init_model(7, M, 3)
    model = tmp_path / "m.hmm"
    e.hmm.save_model(model, "m", pi, A, B)
    seqs = [e.formats.read_seq(f)[2] for f in files]
    vit = e.hmm.viterbi(pi, A, B, seqs[:5])
    fwd = e.hmm.score([(pi, A, B)], seqs[:5])["log_prob"][:, 0]
    for full in (False, True):
        out = _cli("-P", "-Q", "--hmm", str(model), *(["--full"] if full else []), *files).splitlines()
        plain = _cli(*(["--full"] if full else []), *files).splitlines()
        k = 0
        for s, f in enumerate(files):
            assert out[k] == plain[s]  # the symbol line as `seq show` prints it
            k += 1
            if s == 5:  # M differs from the model's
                assert out[k] == f"  codebook size M={M + 1} differs from the model's M={M}: no log_prob, no q_opt"
                k += 1
                continue
            assert out[k].startswith("  log_prob = ") and _bits(float(out[k].split(" = ")[1])) == _bits(fwd[s])
            k += 1
            if s == 4:  # a symbol >= M: no path, -inf, a note
                assert out[k] == "  q_opt_log_prob = -inf"
                assert out[k + 1] == f"  note: symbol {M + 3} at t = 2 is outside the model's alphabet (M = {M})"
                k += 2
                continue
            assert out[k] == "  q_opt = " + R.abbreviated(vit["path"][s], full), (s, full)
            assert (", ..., " in out[k]) == (not full and len(seqs[s]) > 30)
            assert _bits(float(out[k + 1].split("  q_opt_log_prob = ")[1])) == _bits(vit["log_prob"][s])
            k += 2
        assert k == len(out)
    # -c -Q: only the new lines
    out = _cli("-c", "-Q", "--hmm", str(model), *files[:3]).splitlines()
    assert len(out) == 6 and all(l.startswith("  q_opt") for l in out)
    assert _cli("-L", "-P", "--hmm", str(model), files[0]).splitlines()[0] == "7"


_CHILD = r"""
import sys
import ecoz2rs_amd as e
from ecoz2rs_amd._lib import check
files, kw = sys.argv[5:], [int(x) for x in sys.argv[1:4]]
arr, _k = e.hmm._strs(files)
check(e.lib.ecoz2_seq_show_files(kw[0], kw[1], kw[2], sys.argv[4].encode(), arr, len(files)))
"""


def test_reference_entry_point_prints_what_the_cli_prints(tmp_path):
    files = _files(tmp_path)
    e.hmm.set_random_seed(6)
    model = tmp_path / "m.hmm"
    e.hmm.save_model(model, "m", *e.hmm.init_model(70, 16, 0))
    env = dict(os.environ, PYTHONPATH=ROOT)
    for with_prob, gen_q, no_seq in ((1, 1, 0), (0, 1, 1), (1, 0, 0)):
        flags = (["-P"] if with_prob else []) + (["-Q"] if gen_q else []) + (["-c"] if no_seq else [])
        cli = _cli(*flags, "--hmm", str(model), *files)
        r = subprocess.run([sys.executable, "-c", _CHILD, str(with_prob), str(gen_q), str(no_seq), str(model), *files],
                           capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        assert r.stdout == cli, flags


def test_cli_chain_cascade_paths_do_not_go_back(tmp_path):
    """vq learn -> vq quantize -> hmm learn -t 3 -> seq show -Q: the cascade model only moves forward"""
    env = dict(os.environ, NO_COLOR="1", ECOZ2_VQ_MAX_CODEBOOK_SIZE="32")
    for k in ("ECOZ2_VQ_OUT_ROOT", "ECOZ2_VQ_QUIET"):
        env.pop(k, None)

    def run(*args):
        r = subprocess.run([EXE, *args], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    classes, _files = _corpus(tmp_path, 2, 5, 2, seed=9, phones=8, string_len=4)
    run("vq", "learn", "-P", "36", "--predictors", "tt.csv")
    run("vq", "quantize", "--codebook", "data/codebooks/_/eps_0.05_M_0032.cbook", "--predictors", "data/predictors")
    run("hmm", "learn", "-N", "5", "-M", "32", "-t", "3", "-s", "3", "-I", "6", "--class-name", classes[0], "--sequences", "tt.csv")
    seq_dir = tmp_path / "data" / "sequences" / "M32" / classes[0]
    seqs = sorted(str(p) for p in seq_dir.glob("*.seq"))
    assert len(seqs) == 7
    out = run("seq", "show", "-c", "-Q", "--full", "--hmm", f"data/hmms/N5__M32_t3__a0.3_I6/{classes[0]}.hmm", *seqs).splitlines()
    paths = [[int(x) for x in l.split(" = ")[1].split(", ")] for l in out if l.startswith("  q_opt = ")]
    lps = [float(l.split(" = ")[1]) for l in out if l.startswith("  q_opt_log_prob = ")]
    assert len(paths) == 7 and len(lps) == 7 and all(np.isfinite(lps))
    for p, f in zip(paths, seqs):
        assert len(p) == len(e.formats.read_seq(f)[2]) and p[0] == 0
        assert all(b - a in (0, 1, 2) for a, b in zip(p, p[1:])), p  # cascade-3: stay, or one or two states on
