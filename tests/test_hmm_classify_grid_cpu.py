"""`hmm classify --grid`, CPU side: the argument checks of e2vq_hmm_classify_grid / e2vq_hmm_score_grid
and of the CLI run before any HIP call (so they answer the same with or without a device) and write no file; the usage
text names the new form; k_hmm_score_grid is in the gfx950 build without scratch or spilled registers, with its
cross-lane reads and within its register budget.  The GPU parity tests are in test_gpu_hmm_classify_grid.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXE = os.path.join(CSRC, "ecoz2")


def _err():
    return e.lib.e2vq_last_error().decode()


def _model(path, cls, N, M):
    path.parent.mkdir(parents=True, exist_ok=True)
    hmm.save_model(path, cls, np.full(N, 1.0 / N), np.full((N, N), 1.0 / N), np.full((N, M), 1.0 / M))
    return str(path)


def _seq(path, cls, M, n=10):
    path.parent.mkdir(parents=True, exist_ok=True)
    e.formats.write_seq(str(path), cls, M, np.arange(n) % M)
    return str(path)


@pytest.fixture
def corpus(tmp_path):
    """models of classes A and B at (3, 16), of A at (5, 16) and (3, 32); sequences of A and B at M = 16, of A at 32"""
    models = [_model(tmp_path / "hmms" / f"N{N}__M{M}" / f"{c}.hmm", c, N, M)
              for N, M, c in ((3, 16, "A"), (3, 16, "B"), (5, 16, "A"), (3, 32, "A"))]
    seqs = [_seq(tmp_path / "seqs" / f"M{M}" / c / f"{k}.seq", c, M) for M, c in ((16, "B"), (16, "A"), (32, "A")) for k in range(2)]
    return tmp_path, models, seqs


def _classify_grid(models, seqs, cdir=None, summary=None):
    m, _k1 = hmm._strs(models)
    s, _k2 = hmm._strs(seqs)
    return e.lib.e2vq_hmm_classify_grid(m, len(models), s, len(seqs), 0, str(cdir).encode() if cdir else None,
                                        str(summary).encode() if summary else None)


@pytest.mark.parametrize("case,needle", [
    ("no_models", "e2vq_hmm_classify_grid: no models"),
    ("no_sequences", "e2vq_hmm_classify_grid: no sequences"),
    ("dup_class", "grid point N=3 M=16: class 'A' has more than one model"),
    ("point_without_sequences", "grid point N=4 M=64: no sequence with codebook size 64 among the given ones"),
    ("sequence_without_model", "no model with codebook size 48 among the given ones"),
])
def test_classify_grid_refuses_before_the_device(corpus, case, needle):
    tmp_path, models, seqs = corpus
    if case == "no_models":
        models = []
    elif case == "no_sequences":
        seqs = []
    elif case == "dup_class":
        models = models + [_model(tmp_path / "other" / "A.hmm", "A", 3, 16)]
    elif case == "point_without_sequences":
        models = models + [_model(tmp_path / "other" / "A64.hmm", "A", 4, 64)]
    else:
        seqs = seqs + [_seq(tmp_path / "seqs" / "M48" / "A" / "0.seq", "A", 48)]
    out = tmp_path / "out"
    rc = _classify_grid(models, seqs, out / "c12n", out / "summary.csv")
    assert rc == 1 and needle in _err(), _err()
    assert not out.exists()


def _score_grid_rc(Ns=(3, 4), Ms=(8, 8), ranges=((0, 2), (1, 4)), out_offs=None, S=4, K=None, sym_max=0, param_offs=None):
    K = len(Ns) if K is None else K
    sizes = [n + n * n + n * m for n, m in zip(Ns, Ms)]
    if param_offs is None:
        param_offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]) if sizes else []
    params = np.full(max(sum(max(s, 1) for s in sizes), 1) * 2, 0.5)
    sym = np.zeros(4 * S, dtype=np.uint16)
    sym[0] = sym_max
    offs = np.arange(S + 1, dtype=np.int64) * 4
    ns, ms = np.array(Ns, dtype=np.int32), np.array(Ms, dtype=np.int32)
    po = np.array(param_offs, dtype=np.int64)
    lo = np.array([r[0] for r in ranges], dtype=np.int64)
    hi = np.array([r[1] for r in ranges], dtype=np.int64)
    if out_offs is None:
        out_offs = np.concatenate([[0], np.cumsum(np.abs(hi - lo))[:-1]]) if len(lo) else []
    oo = np.array(out_offs, dtype=np.int64)
    n = 64
    mant, ex, st, lp = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32), np.zeros(n)
    return e.lib.e2vq_hmm_score_grid(0, K, ns.ctypes.data, ms.ctypes.data, params.ctypes.data, po.ctypes.data, sym.ctypes.data,
                                     offs.ctypes.data, S, lo.ctypes.data, hi.ctypes.data, oo.ctypes.data, mant.ctypes.data,
                                     ex.ctypes.data, st.ctypes.data, lp.ctypes.data)


@pytest.mark.parametrize("kw,needle", [
    (dict(K=0, Ns=(), Ms=(), ranges=()), "e2vq_hmm_score_grid: bad arguments (K = 0)"),
    (dict(Ns=(3, 0)), "model 1: HMM with N=0 M=8 out of range"),
    (dict(Ns=(513, 3)), "model 0: HMM with N=513 M=8 out of range"),
    (dict(Ms=(8, 0)), "model 1: HMM with N=4 M=0 out of range"),
    (dict(Ms=(65537, 8)), "model 0: HMM with N=3 M=65537 out of range"),
    (dict(ranges=((0, 2), (2, 2))), "model 1: sequence range [2, 2) not a non-empty part of [0, 4)"),
    (dict(ranges=((3, 1), (0, 4))), "model 0: sequence range [3, 1) not a non-empty part of [0, 4)"),
    (dict(ranges=((-1, 2), (0, 4))), "model 0: sequence range [-1, 2) not a non-empty part of [0, 4)"),
    (dict(ranges=((0, 2), (1, 5))), "model 1: sequence range [1, 5) not a non-empty part of [0, 4)"),
    (dict(out_offs=(0, 1)), "output ranges overlap: [0, 2) and [1, 4)"),
    (dict(out_offs=(2, 0)), "output ranges overlap: [0, 3) and [2, 4)"),
    (dict(out_offs=(0, -2)), "model 1: output offset -2 < 0"),
    (dict(param_offs=(0, -1)), "model 1: parameter offset -1 < 0"),
])
def test_score_grid_refuses_before_the_device(kw, needle):
    assert _score_grid_rc(**kw) == 1
    assert needle in _err(), _err()


def test_python_score_grid_checks_the_range_count():
    with pytest.raises(ValueError):
        hmm.score_grid([(np.ones(2) / 2, np.ones((2, 2)) / 2, np.ones((2, 4)) / 4)], [np.zeros(3, np.uint16)], [(0, 1), (0, 1)])


# ---- CLI ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def cli_tree(tmp_path):
    for M, classes in ((16, ("C0", "C1")), (33, ("C0",))):
        for c in classes:
            _model(tmp_path / "data" / "hmms" / f"N3__M{M}_t3__a0.3" / f"{c}.hmm", c, 3, M)
            for k in range(2):
                _seq(tmp_path / "data" / "sequences" / f"M{M}" / c / f"{k:05d}.seq", c, M, 12)
    (tmp_path / "tt.csv").write_text("tt,class,selection\nTEST,C0,00000\nTEST,C0,00001\nTEST,C1,00000\n")
    return tmp_path


def _cli(root, *args):
    r = subprocess.run([EXE, "hmm", "classify", *args], cwd=root, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


_BASE = ["--grid", "--models", "data/hmms", "--tt", "TEST", "-c", "out/c12n", "--summary", "out/summary.csv"]


@pytest.mark.parametrize("args,code,needle", [
    (["--class-name", "C0", "-M", "16", "--sequences", "tt.csv"], 2, "--grid and --class-name exclude each other"),
    (["--predictors", "x.prd", "-M", "16", "--sequences", "tt.csv"], 2, "--grid and --predictors exclude each other"),
    (["--codebooks", "x.cbook", "-M", "16", "--sequences", "tt.csv"], 2, "--grid and --codebooks exclude each other"),
    (["--sequences", "tt.csv"], 2, "--grid with a tt.csv needs -M <m1,m2,...>"),
    (["-M", "16,x", "--sequences", "tt.csv"], 2, "comma-separated integers"),
    (["-M", "16,33,16", "--sequences", "tt.csv"], 2, "-M 16: given more than once"),
    (["-M", "0,16", "--sequences", "tt.csv"], 2, "-M 0: not a codebook size"),
    (["-M", "64", "--sequences", "data/sequences"], 0, "No models given"),
    (["-M", "16", "--sequences", "data/sequences/M33"], 0, "No sequences given"),
    (["--sequences", "data/sequences/M16"], 0, "grid point N=3 M=33: no sequence with codebook size 33 among the given ones"),
])
def test_cli_grid_refusals(cli_tree, args, code, needle):
    rc, out, err = _cli(cli_tree, *_BASE, *args)
    assert rc == code and needle in (err if code == 2 else out), (rc, out, err)
    assert not (cli_tree / "out").exists()


def test_cli_refuses_a_sequence_without_a_model(cli_tree):
    _seq(cli_tree / "data" / "sequences" / "M48" / "C0" / "00000.seq", "C0", 48)
    rc, out, err = _cli(cli_tree, *_BASE, "--sequences", "data/sequences")
    assert rc == 0 and "no model with codebook size 48 among the given ones" in out, (rc, out, err)
    assert not (cli_tree / "out").exists()


def test_cli_usage_names_the_grid(cli_tree):
    rc, _out, err = _cli(cli_tree, *_BASE, "--class-name", "C0", "-M", "16", "--sequences", "tt.csv")
    assert rc == 2 and "ecoz2 hmm classify --grid [-r] [-c|--c12n <dir>] [--summary <file.csv>]" in err


# ---- ISA guard (style of test_isa_guards.py) ---------------------------------------------------------------------------
VGPR_BUDGET = 64  # 8 waves a SIMD, so that the 4-wave groups of a CU's worth of packs stay resident


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_device.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_device.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _kernel(text):
    names = re.findall(r"^(\S*k_hmm_score_grid\S*):", text, re.M)
    names = [n for n in names if not n.startswith(".")]
    assert len(names) == 1, names
    body = text[text.index("\n" + names[0] + ":"):]
    return names[0], body[:body.index("s_endpgm")]


def test_score_grid_kernel_has_no_scratch_no_spill_and_fits_its_budget(asm):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if "k_hmm_score_grid" in m.group(1)]
    assert len(metas) == 1
    g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")


def test_score_grid_kernel_reads_across_lanes(asm):
    _name, body = _kernel(asm)
    assert re.search(r"\bds_bpermute_b32\b|_dpp\b", body), "no cross-lane read in k_hmm_score_grid"
    assert "ds_read_b64" in body or "ds_read2_b64" in body or "ds_load_b64" in body
