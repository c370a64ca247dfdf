"""HMM Viterbi decoding, CPU side: the numpy restatement against a literal transcription of the
contract and against brute force, the C-ABI and CLI surface that needs no GPU (declarations, exports, argument
errors, model checks), and an ISA guard on the wave kernel.  The GPU parity tests are in test_gpu_hmm_viterbi.py."""
import ctypes as C
import itertools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from tests import hmm_viterbi_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _models(N, M, seed):
    """random, uniform (every comparison a tie) and the two cascades (zeros in pi and A: -inf in the sums)"""
    e.hmm.set_random_seed(seed)
    return [e.hmm.init_model(N, M, t) for t in range(4)]


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("N,M", [(1, 4), (2, 3), (5, 16), (9, 64)])
def test_restatement_equals_transcription(N, M):
    rng = np.random.default_rng(N * 100 + M)
    seqs = [rng.integers(0, M, n).astype(np.uint16) for n in (0, 1, 2, 7, 40)]
    seqs.append(np.array([0, 1, M, 2], dtype=np.uint16))  # a symbol outside the alphabet: status 2
    for k, (pi, A, B) in enumerate(_models(N, M, 11 + N)):
        if k == 3 and N >= 3:
            B = B.copy()
            B[:, 0] = 0.0  # symbol 0 cannot be emitted: -inf from the emissions too
            seqs.append(np.array([1, 0, 2], dtype=np.uint16))
        got = R.viterbi(pi, A, B, seqs)
        for s, sq in enumerate(seqs):
            path, lp, st = R.transcribe(pi, A, B, sq)
            assert got["path"][s].tolist() == path, (k, s)
            assert _same(got["log_prob"][s], lp) and got["status"][s] == st, (k, s)
    # the uniform model: every state ties, the lowest index wins everywhere
    pi, A, B = _models(N, M, 3)[1]
    got = R.viterbi(pi, A, B, [rng.integers(0, M, 12).astype(np.uint16)])
    assert got["path"][0].tolist() == [0] * 12 and got["status"][0] == 0


@pytest.mark.parametrize("N", [1, 2, 3])
def test_restatement_matches_brute_force(N):
    rng = np.random.default_rng(40 + N)
    M = 4
    checked_paths = 0
    for trial in range(12):
        e.hmm.set_random_seed(500 + 13 * N + trial)
        pi, A, B = e.hmm.init_model(N, M, [0, 0, 2, 3][trial % 4])
        lpi, lA, lB = R.log_model(pi, A, B)
        for T in range(1, 7):
            sq = rng.integers(0, M, T)
            scores = []
            for q in itertools.product(range(N), repeat=T):
                v = lpi[q[0]] + lB[q[0], sq[0]]
                for t in range(1, T):
                    v = v + lA[q[t - 1], q[t]] + lB[q[t], sq[t]]
                scores.append((v, q))
            best = max(v for v, _ in scores)
            path, lp, st = R.viterbi_logs(lpi, lA, lB, sq)
            if best == -math.inf:
                assert lp == -math.inf and st == 1
                continue
            assert abs(lp - best) <= 1e-12 * max(1.0, abs(best)) and st == 0
            near = [q for v, q in scores if v > best - 1e-9 * max(1.0, abs(best))]
            if len(near) == 1:  # a unique best path: it is the one found
                assert tuple(path.tolist()) == near[0]
                checked_paths += 1
    assert checked_paths > 20


def _decl(header, name):
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def test_header_declares_seq_show_files_in_the_reference_order():
    header = open(os.path.join(ROOT, "include", "ecoz2_classify.h")).read()
    # src/ecoz2_lib/mod.rs:169-177, with the third argument named after what the reference's caller passes there
    assert _decl(header, "ecoz2_seq_show_files") == [
        "int with_prob", "int gen_q_opt", "int no_sequence", "const char *hmm_filename",
        "const char *const *sequence_filenames", "int num_sequences"]
    assert _decl(header, "e2vq_seq_show_files")[:6] == _decl(header, "ecoz2_seq_show_files")
    assert _decl(header, "e2vq_seq_show_files")[6:] == ["int full", "int only_length"]
    assert _decl(header, "e2vq_hmm_viterbi") == [
        "int device", "int N", "int M", "const double *pi", "const double *A", "const double *B", "const uint16_t *sym",
        "const int64_t *offs", "int S", "uint16_t *path", "double *log_prob", "int *status"]


@pytest.mark.skipif(shutil.which("nm") is None, reason="nm not installed")
def test_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", e.lib_path], capture_output=True, text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert {"ecoz2_seq_show_files", "e2vq_seq_show_files", "e2vq_hmm_viterbi"} <= names


def test_model_checks_come_before_the_device():
    pi, A, B = e.hmm.init_model(3, 4, 0)
    seqs = [np.array([0, 1, 2], dtype=np.uint16)]
    for bad, where in ((-0.5, "pi"), (np.nan, "A"), (np.inf, "B")):
        p2, A2, B2 = pi.copy(), A.copy(), B.copy()
        {"pi": p2, "A": A2, "B": B2}[where].flat[1] = bad
        with pytest.raises(e.Ecoz2Error, match=r"HMM parameter " + where + r"\[1\] = .*not a finite non-negative number"):
            e.hmm.viterbi(p2, A2, B2, seqs)
    with pytest.raises(e.Ecoz2Error, match="out of range"):
        e.hmm.viterbi(np.ones(513) / 513, np.ones((513, 513)) / 513, np.ones((513, 2)) / 2, seqs)


def _write_seqs(tmp_path, M=8):
    rng = np.random.default_rng(3)
    files = []
    for k, n in enumerate((5, 31, 0)):
        f = tmp_path / f"s{k}.seq"
        e.formats.write_seq(str(f), "Cx", M, rng.integers(0, M, n).astype(np.uint16))
        files.append(str(f))
    return files


def test_cli_argument_errors_and_unchanged_output(tmp_path):
    files = _write_seqs(tmp_path)
    pi, A, B = e.hmm.init_model(3, 8, 1)
    model = tmp_path / "m.hmm"
    e.hmm.save_model(model, "Cx", pi, A, B)
    run = lambda *a: subprocess.run([EXE, "seq", "show", *a], capture_output=True, text=True, timeout=60)
    for flags in (["-P"], ["-Q"], ["-P", "-Q", "-c"]):
        r = run(*flags, *files)
        assert r.returncode == 2 and "--hmm" in r.stderr and r.stdout == ""
        r = run(*flags, "--hmm", str(model), "--pickle", str(tmp_path / "o.pkl"), "-M", "8", "--tt", "TRAIN", *files)
        assert r.returncode == 2 and "--pickle" in r.stderr and not os.path.exists(tmp_path / "o.pkl")
    # without -P / -Q, --hmm changes nothing, and the output is the symbol line of Sequence::show
    for extra in ([], ["-c"], ["-L"], ["--full"]):
        plain = run(*extra, *files)
        assert plain.returncode == 0 and run(*extra, "--hmm", str(model), *files).stdout == plain.stdout
    lines = run(*files).stdout.splitlines()
    syms = [e.formats.read_seq(f)[2] for f in files]
    assert lines[0] == f"<Cx(M=8,L=5): {R.abbreviated(syms[0], False)}>"
    assert lines[1] == f"<Cx(M=8,L=31): {R.abbreviated(syms[1], False)}>" and ", ..., " in lines[1]
    assert lines[2] == "<Cx(M=8,L=0): >"
    assert run("-L", *files).stdout == "5\n31\n0\n" and run("-c", *files).stdout == ""


def test_without_a_device_viterbi_fails(tmp_path):
    if e.lib.e2vq_device_count() > 0:
        pytest.skip("a HIP device is present")
    pi, A, B = e.hmm.init_model(3, 8, 3)
    with pytest.raises(e.Ecoz2Error, match="no HIP device"):
        e.hmm.viterbi(pi, A, B, [np.array([0, 1], dtype=np.uint16)])
    files = _write_seqs(tmp_path)
    model = tmp_path / "m.hmm"
    e.hmm.save_model(model, "Cx", pi, A, B)
    r = subprocess.run([EXE, "seq", "show", "-Q", "--hmm", str(model), *files], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "no HIP device" in r.stdout
    with pytest.raises(e.Ecoz2Error, match="no HIP device"):
        e.hmm.seq_show_files(True, False, False, model, files)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_isa_viterbi_kernels_have_no_scratch(tmp_path):
    from tests.test_isa_guards import FLAGS, Kernel

    out = tmp_path / "hmm_viterbi.s"
    subprocess.run([HIPCC, *FLAGS, "-o", str(out), os.path.join(ROOT, "ecoz2rs_amd", "csrc", "hmm_viterbi.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    for pattern in (r"13k_hmm_viterbiILb1E", r"13k_hmm_viterbiILb0E", r"16k_hmm_viterbi_wgILb1E", r"15k_hmm_backtrack"):
        k = Kernel(text, pattern)
        assert k.scratch == 0 and k.spill == 0, (k.name, k.scratch, k.spill)
        assert k.vgpr <= 64, (k.name, k.vgpr)  # (8 waves per SIMD)
    # the wave kernel's step: adds and compares only, the state broadcast by readlane
    k = Kernel(text, r"13k_hmm_viterbiILb1E")
    assert k.count("v_readlane_b32") >= 2 and k.count("v_cmp_gt_f64") >= 1
    assert not any(m in l for l in k.body for m in ("v_rcp_f64", "v_div_scale_f64", "v_fma_f64"))
