"""`hmm scan`, CPU side: the argument checks of e2vq_hmm_scan / e2vq_hmm_scan_files and of the CLI run
before any HIP call (so they answer the same with or without a device) and write no file; the window arithmetic; the CSV
and stdout block of e2vq_hmm_scan_report on a hand-made result; the usage text names the command; k_hmm_scan,
k_hmm_scan_wg and k_scan_top2 are in the gfx950 build without scratch or spilled registers.  The GPU parity tests are in
test_gpu_hmm_scan.py.  For test_gpu_hmm_scan_shapes.py: the restated plan of scan_device (tests/hmm_scan_cases.py) against
the sources, the cap, span, runs and bytes of every row of SCAN_SHAPES, that every launch stages all its longest run covers
(which the earlier span formula does not at hops near 2^63), and on the oracle alone which windows of the event cases get
which status."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from ecoz2rs_amd import hmm

from . import hmm_scan_cases as cases
from . import lpc_wavs
from . import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ecoz2rs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXE = os.path.join(CSRC, "ecoz2")


def _err():
    return e.lib.e2vq_last_error().decode()


def _uniform(N, M):
    return np.full(N, 1.0 / N), np.full((N, N), 1.0 / N), np.full((N, M), 1.0 / M)


# ---- e2vq_hmm_scan: refusals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,needle", [
    (dict(window=0), "e2vq_hmm_scan: window of 0 frames (at least 1)"),
    (dict(window=-3), "e2vq_hmm_scan: window of -3 frames (at least 1)"),
    (dict(hop=0), "e2vq_hmm_scan: hop of 0 frames (at least 1)"),
    (dict(hop=-1), "e2vq_hmm_scan: hop of -1 frames (at least 1)"),
    (dict(Ns=()), "e2vq_hmm_scan: 0 models (at least 1)"),
    (dict(Ns=(3, 0)), "e2vq_hmm_scan: model 1 has N=0 states (1 .. 512)"),
    (dict(Ns=(513,)), "e2vq_hmm_scan: model 0 has N=513 states (1 .. 512)"),
])
def test_scan_refuses_before_the_device(kw, needle):
    Ns = kw.pop("Ns", (3,))
    models = [_uniform(max(N, 1), 8) for N in Ns]
    if Ns and min(Ns) < 1:  # (an N the arrays cannot have: the C call directly)
        K = len(Ns)
        ns = (C.c_int * K)(*Ns)
        ptr = lambda i: (C.c_void_p * K)(*[np.ascontiguousarray(m[i]).ctypes.data for m in models])
        sym, offs = np.zeros(8, np.uint16), np.array([0, 8], np.int64)
        rc = e.lib.e2vq_hmm_scan(0, K, ns, 8, ptr(0), ptr(1), ptr(2), sym.ctypes.data, offs.ctypes.data, 1, 4, 4, *([None] * 9), 0)
        assert rc == 1 and needle in _err(), _err()
        return
    with pytest.raises(e.Ecoz2Error) as ei:
        hmm.scan(models, np.zeros(8, np.uint16), [0, 8], kw.get("window", 4), kw.get("hop", 2))
    assert needle in str(ei.value)


# ---- window arithmetic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,L,H,W", [
    (9, 10, 1, 0),     # T < L
    (10, 10, 1, 1),    # T == L
    (10, 10, 7, 1),
    (30, 4, 9, 3),     # H > L: windows at 0, 9, 18 (27 + 4 > 30)
    (31, 4, 9, 4),     # ... and at 27
    (25, 10, 4, 4),    # a dropped tail: 0, 4, 8, 12 (16 + 10 > 25)
    (26, 10, 4, 5),
    (0, 1, 1, 0),
    (5, 1, 1, 5),
    (38265, 100, 1, 38166),
    (38265, 100, 10, 3817),
])
def test_window_count(T, L, H, W):
    assert list(hmm.scan_windows([0, T], L, H)) == [0, W]
    assert W == len([i for i in range(0, T, H) if i + L <= T])


def test_window_offsets_of_several_streams():
    offs = np.cumsum([0, 3, 10, 0, 25, 9])
    assert list(hmm.scan_windows(offs, 10, 4)) == [0, 0, 1, 1, 5, 5]
    with pytest.raises(e.Ecoz2Error):
        hmm.scan_windows(offs, 0, 4)
    with pytest.raises(e.Ecoz2Error):
        hmm.scan_windows(offs, 4, 0)


# ---- e2vq_hmm_scan_files: refusals -----------------------------------------------------------------------------------------
@pytest.fixture
def corpus(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    models = []
    for c, N in (("A", 3), ("B", 5)):
        hmm.save_model(d / f"{c}.hmm", c, *_uniform(N, 16))
        models.append(str(d / f"{c}.hmm"))
    hmm.save_model(d / "C32.hmm", "C", *_uniform(3, 32))
    rng = np.random.default_rng(1)
    e.formats.write_cbook(str(d / "m16p4.cbook"), "_", rng.uniform(-0.5, 0.5, (16, 5)))
    e.formats.write_cbook(str(d / "m32p4.cbook"), "_", rng.uniform(-0.5, 0.5, (32, 5)))
    e.formats.write_cbook(str(d / "m16p6.cbook"), "_", rng.uniform(-0.5, 0.5, (16, 7)))
    e.formats.write_prd(str(d / "x.prd"), "A", rng.uniform(0.1, 1.0, (40, 5)))
    e.formats.write_seq(str(d / "x.seq"), "A", 16, np.arange(40) % 16)
    e.formats.write_seq(str(d / "y32.seq"), "A", 32, np.arange(40) % 32)
    lpc_wavs.write_wav(d / "x.wav", lpc_wavs.to_pcm(lpc_wavs.ar_source(3, 4, 4000, 0.5), 16), 8000, 16)
    (d / "notes.txt").write_text("x")
    return tmp_path, d, models


def _scan_files(models, inputs, out, codebook=None, P=4, window=8, hop=4):
    m, _k1 = hmm._strs(models)
    f, _k2 = hmm._strs(inputs)
    return e.lib.e2vq_hmm_scan_files(m, len(models), str(codebook).encode() if codebook else None, f, len(inputs), P, 45, 15, window,
                                     hop, 0.0, str(out).encode())


@pytest.mark.parametrize("case,needle", [
    ("no_models", "e2vq_hmm_scan_files: no models"),
    ("no_inputs", "e2vq_hmm_scan_files: no inputs"),
    ("window", "e2vq_hmm_scan_files: window of 0 frames (at least 1)"),
    ("hop", "e2vq_hmm_scan_files: hop of 0 frames (at least 1)"),
    ("models_M", "model has M=32 but"),
    ("cb_M", "codebook has M=32 but the models have M=16"),
    ("cb_P_prd", "x.prd: prediction order 4 differs from the codebook's 6"),
    ("cb_P_wav", "x.wav: prediction order -P 4 differs from the codebook's 6"),
    ("seq_M", "y32.seq: codebook size 32 differs from the models' 16"),
    ("no_codebook", "signals and predictors need a codebook"),
    ("extension", "notes.txt: not a .wav, .prd or .seq file"),
    ("same_csv", "would both write"),
])
def test_scan_files_refuses_before_the_device(corpus, case, needle):
    tmp_path, d, models = corpus
    kw = dict(codebook=d / "m16p4.cbook")
    inputs = [str(d / "x.seq")]
    if case == "no_models":
        models = []
    elif case == "no_inputs":
        inputs = []
    elif case == "window":
        kw["window"] = 0
    elif case == "hop":
        kw["hop"] = 0
    elif case == "models_M":
        models = models + [str(d / "C32.hmm")]
    elif case == "cb_M":
        kw["codebook"] = d / "m32p4.cbook"
        inputs = [str(d / "x.prd")]
    elif case == "cb_P_prd":
        kw["codebook"] = d / "m16p6.cbook"
        inputs = [str(d / "x.prd")]
    elif case == "cb_P_wav":
        kw["codebook"] = d / "m16p6.cbook"
        inputs = [str(d / "x.wav")]
    elif case == "seq_M":
        inputs = [str(d / "x.seq"), str(d / "y32.seq")]
    elif case == "no_codebook":
        kw["codebook"] = None
        inputs = [str(d / "x.prd")]
    elif case == "extension":
        inputs = [str(d / "notes.txt")]
    else:
        inputs = [str(d / "x.seq"), str(d / "x.prd")]
    out = tmp_path / "out"
    assert _scan_files(models, inputs, out, **kw) == 1
    assert needle in _err(), _err()
    assert not out.exists()


# ---- the report: CSV and stdout block of a hand-made result ---------------------------------------------------------------
def _report(tmp_path, capfd, best, lp1, second, lp2, min_margin, names=("whale", "noise", "ship"), L=100, H=10, T=1000):
    names_c, _k = hmm._strs(names)
    best, second = np.array(best, np.int32), np.array(second, np.int32)
    lp1, lp2 = np.array(lp1, np.float64), np.array(lp2, np.float64)
    csv = tmp_path / "rep" / "x.csv"
    capfd.readouterr()
    rc = e.lib.e2vq_hmm_scan_report(b"x.wav", T, len(names), names_c, len(best), L, H, 45, 15, best.ctypes.data, lp1.ctypes.data,
                                    second.ctypes.data, lp2.ctypes.data, min_margin, str(csv).encode())
    assert rc == 0, _err()
    return csv.read_text().split("\n"), capfd.readouterr().out.split("\n")


def test_report_csv_and_runs(tmp_path, capfd):
    inf = float("inf")
    best = [0, 0, 1, 1, 1, 2, 0]
    lp1 = [-10.5, -11.0, -9.0, -9.25, -1 / 3, -inf, -7.0]
    second = [1, 1, 0, 0, 2, 1, 2]
    lp2 = [-12.5, -11.5, -9.5, -12.0, -8.0, -inf, -inf]
    rows, out = _report(tmp_path, capfd, best, lp1, second, lp2, 1.0)
    assert rows[0] == "window,begin_frame,end_frame,begin_s,end_s,class,log_prob,second_class,second_log_prob"
    # window 2: frames [20, 120); begin 20 x 15 ms; end = (119 x 15 + 45) ms
    assert rows[3] == "2,20,120,0.29999999999999999,1.8300000000000001,noise,-9,whale,-9.5"
    assert rows[5] == "4,40,140,0.59999999999999998,2.1299999999999999,noise,%.17g,ship,-8" % (-1 / 3)
    assert rows[6] == "5,50,150,0.75,2.2799999999999998,,-inf,,-inf"      # no model can emit the window
    assert rows[7] == "6,60,160,0.90000000000000002,2.4300000000000002,whale,-7,,-inf"
    assert rows[8] == "" and len(rows) == 9
    assert out[0] == "x.wav: T=1000  windows=7  (window 100 frames, hop 10)"
    assert out[1:5] == ["  'whale': 3", "  'noise': 3", "  'ship': 0", "  (no model can emit the window): 1"]
    assert out[5] == "  runs (margin >= 1):"
    # margins: 2, 0.5, 0.5, 2.75, 7.67, -, inf
    assert out[6:9] == ["    0.000 - 1.530 whale", "    0.450 - 2.130 noise", "    0.900 - 2.430 whale"]
    assert out[9].endswith("x.csv saved")
    _rows, out0 = _report(tmp_path, capfd, best, lp1, second, lp2, 0.0)
    assert out0[6:9] == ["    0.000 - 1.680 whale", "    0.300 - 2.130 noise", "    0.900 - 2.430 whale"]


def test_report_with_one_model(tmp_path, capfd):
    rows, out = _report(tmp_path, capfd, [0, 0], [-3.0, -4.0], [-1, -1], [-float("inf")] * 2, 5.0, names=("only",), L=4, H=4, T=8)
    assert rows[1] == "0,0,4,0,0.089999999999999997,only,-3,,-inf"
    assert out[3] == "    0.000 - 0.150 only"


def test_report_refuses_a_model_index_out_of_range(tmp_path):
    names_c, _k = hmm._strs(["a"])
    best, second, lp = np.array([1], np.int32), np.array([-1], np.int32), np.zeros(1)
    rc = e.lib.e2vq_hmm_scan_report(b"x", 4, 1, names_c, 1, 4, 4, 45, 15, best.ctypes.data, lp.ctypes.data, second.ctypes.data,
                                    lp.ctypes.data, 0.0, str(tmp_path / "no.csv").encode())
    assert rc == 1 and "names a model outside [0, 1)" in _err()
    assert not (tmp_path / "no.csv").exists()


# ---- CLI -----------------------------------------------------------------------------------------------------------------
def _cli(cwd, *args):
    r = subprocess.run([EXE, "hmm", "scan", *args], cwd=cwd, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("args,code,needle", [
    (["--sequences", "in/x.seq", "--window", "8"], 2, "--models <files|dirs>... is required"),
    (["--models", "in/A.hmm", "--window", "8"], 2, "exactly one of --signals, --predictors and --sequences"),
    (["--models", "in/A.hmm", "--window", "8", "--sequences", "in/x.seq", "--predictors", "in/x.prd"], 2, "exactly one of"),
    (["--models", "in/A.hmm", "--sequences", "in/x.seq"], 2, "--window <frames> is required"),
    (["--models", "in/A.hmm", "--sequences", "in/x.seq", "--window", "8", "--hop", "-2"], 2, "--hop -2: at least 1"),
    (["--models", "in/A.hmm", "--signals", "in/x.wav", "--window", "8"], 2, "--signals and --predictors need --codebook"),
    (["--models", "in/A.hmm", "in/C32.hmm", "--sequences", "in/x.seq", "--window", "8", "-c", "out"], 1, "model has M=32 but"),
    (["--models", "in/A.hmm", "--sequences", "in/y32.seq", "--window", "8", "-c", "out"], 1, "codebook size 32 differs from the models' 16"),
    (["--models", "in/A.hmm", "--codebook", "in/m16p6.cbook", "-P", "4", "--signals", "in/x.wav", "--window", "8", "-c", "out"], 1,
     "prediction order -P 4 differs from the codebook's 6"),
])
def test_cli_refusals(corpus, args, code, needle):
    tmp_path, _d, _models = corpus
    rc, out, err = _cli(tmp_path, *args)
    assert rc == code and needle in (err if code == 2 else out), (rc, out, err)
    assert not (tmp_path / "out").exists()


def test_usage_names_hmm_scan(tmp_path):
    rc, _out, err = _cli(tmp_path)
    assert rc == 2 and "ecoz2 hmm scan -m|--models <files|dirs>... [--codebook <cbook>] [-P 36] [-W 45] [-O 15] --window <frames>" in err
    assert "--signals <.wav files|dirs>... | --predictors <.prd files|dirs>... | --sequences <.seq files|dirs>..." in err


# ---- ISA guard (style of test_isa_guards.py) ---------------------------------------------------------------------------
VGPR_BUDGET = 64  # eight waves a SIMD, as k_hmm_score_grid


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hmm_scan.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "hmm_scan.hip")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return open(out).read()


def _meta(asm, pattern):
    metas = [m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm, re.S) if re.search(pattern, m.group(1))]
    assert len(metas) == 1, pattern
    return lambda k: int(re.search(r"\." + k + r":\s+(\d+)", metas[0]).group(1))


@pytest.mark.parametrize("pattern", [r"k_hmm_scanILb1E", r"k_hmm_scanILb0E", r"k_hmm_scan_wgE", r"k_scan_top2E"])
def test_scan_kernels_have_no_scratch_no_spill_and_fit_their_budget(asm, pattern):
    g = _meta(asm, pattern)
    assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0
    assert g("vgpr_count") <= VGPR_BUDGET, g("vgpr_count")


def test_scan_kernel_reads_across_lanes_and_from_lds(asm):
    names = [n for n in re.findall(r"^(\S*k_hmm_scanILb1E\S*):", asm, re.M) if not n.startswith(".")]
    assert len(names) == 1, names
    body = asm[asm.index("\n" + names[0] + ":"):]
    body = body[:body.index("s_endpgm")]
    assert re.search(r"\bds_bpermute_b32\b|_dpp\b", body), "no cross-lane read in k_hmm_scan"
    assert "v_readlane_b32" in body, "no wave-uniform read (the one-window-per-wave body) in k_hmm_scan"
    assert re.search(r"ds_(read|load)_u16", body), "the windows' symbols are not read from LDS"


def test_scan_library_exports():
    for name in ("e2vq_hmm_scan", "e2vq_hmm_scan_files", "e2vq_hmm_scan_windows", "e2vq_hmm_scan_report", "e2vq_hmm_scan_last_kernel_ms"):
        assert hasattr(e.lib, name)


# ---- the plan of scan_device, restated (tests/hmm_scan_cases.py), against the sources ----------------------------------------
def _source(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_restated_constants_and_formulas_are_the_sources():
    dev, hip, host = _source("hmm_device.h"), _source("hmm_scan.hip"), _source("hmm_decode.cpp")
    const = lambda text, name: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))
    assert cases.SCAN_SPAN_CAP == const(dev, "SCAN_SPAN_CAP") and cases.SCAN_WAVES == const(hip, "SCAN_WAVES")
    assert cases.SCAN_PACK_MAX_N == const(host, "SCAN_PACK_MAX_N") and cases.WAVE_N == 64
    assert "int scan_waves() { return SCAN_WAVES; }" in hip and "__launch_bounds__(64 * SCAN_WAVES)" in hip
    # the pack width and the rounds, default and clamp
    assert 'if (v && *v) return atoi(v) == 0 || N > 32 ? 1 : e2hmm::WAVE_N / N;' in host
    assert "return N <= SCAN_PACK_MAX_N ? e2hmm::WAVE_N / N : 1;" in host
    assert 'const int r = e2vq_env_int("ECOZ2_HMM_SCAN_ROUNDS", %d);' % cases.SCAN_ROUNDS_DEFAULT in host
    assert "return r < 1 ? 1 : (r > %d ? %d : r);" % (cases.SCAN_ROUNDS_MAX, cases.SCAN_ROUNDS_MAX) in host
    assert [cases.scan_rounds(r) for r in (None, "0", "1", "3", "64", "1000", "-5")] == [4, 1, 1, 3, 64, 64, 1]
    assert [cases.scan_pack_width_in_use(N) for N in (1, 3, 21, 22, 32, 33, 64)] == [64, 21, 3, 1, 1, 1, 1]
    assert [cases.scan_pack_width_in_use(N, "1") for N in (1, 3, 21, 22, 32, 33, 64)] == [64, 21, 3, 2, 2, 1, 1]
    assert [cases.scan_pack_width_in_use(N, "0") for N in (1, 21, 22, 64)] == [1, 1, 1, 1] and cases.scan_pack_width_in_use(22, "") == 1
    # the cap, the runs, and the span of a launch from the runs it makes (no product of the hop with a count across streams)
    assert "i64 cap = (i64)e2hmm::scan_waves() * G * rounds;" in host
    assert "if (window <= e2hmm::SCAN_SPAN_CAP) cap = std::min<i64>(cap, (e2hmm::SCAN_SPAN_CAP - window) / hop + 1);" in host
    assert "runs.push_back(e2hmm::ScanRun{(int)w, (int)std::min<i64>(cap, win_offs[(size_t)s + 1] - w)});" in host
    assert "for (i64 w = win_offs[(size_t)s]; w < win_offs[(size_t)s + 1]; w += cap)" in host
    assert "span = std::max(span, (std::min(cap, n) - 1) * hop + window);" in host
    assert "(int)(span <= e2hmm::SCAN_SPAN_CAP ? span : 0)" in host
    assert "std::min<i64>(cap, W)" not in host
    # the launchers: the bytes, the limits of a launch, and a refusal the caller sees
    assert "const size_t lds = (size_t)N * G * N * 8 + (size_t)span_lds * 2;" in hip
    assert "span_lds < 0 || span_lds > SCAN_SPAN_CAP) return 1;" in hip
    assert hip.count("k0 += %d)" % cases.MODELS_PER_LAUNCH) == 2 and cases.WG_WINDOWS_PER_LAUNCH == 1 << 20
    assert "for (i64 w0 = 0; w0 < W; w0 += 1 << 20) {" in hip and "W - w0 < (1 << 20) ? W - w0 : (1 << 20)" in hip
    for text in (dev, hip):
        assert re.search(r"\bint launch_scan\(", text) and re.search(r"\bint launch_scan_wg\(", text)
        assert not re.search(r"\bvoid launch_scan(_wg)?\(", text)
    assert "if (e2hmm::launch_scan(" in host and "if (e2hmm::launch_scan_wg(" in host


def _plan(name, hop=None, **kw):
    Ns, _M, lens, L, hops = cases.SCAN_SHAPES[name]
    return cases.scan_plan(Ns, lens, L, hops[0] if hop is None else hop, **kw)


def test_every_row_of_the_scan_shapes_shows_the_plan_its_comment_names():
    assert list(cases.SCAN_SHAPES) == ["L8192", "L8191", "L8193", "L4000_H1000", "rounds_N1", "rounds_N21_N64", "many_windows",
                                       "huge_hop_long", "huge_hop_short"]
    pick = lambda p, N, *keys: tuple(p["launches"][N][k] for k in keys)
    # a window of exactly the staging area: one window a run, and the kernel's largest launch at N = 64
    p = _plan("L8192")
    assert p["counts"] == [0, 1, 0, 2]
    for N in (5, 64):
        assert pick(p, N, "cap", "span_lds", "runs") == (1, 8192, [[1], [1, 1]])
    assert p["launches"][64]["lds"] == 49152 == 64 * 64 * 8 + 2 * 8192
    # two windows whose span is exactly 8192, then the one left over
    p = _plan("L8191")
    for N in (21, 64):
        assert pick(p, N, "cap", "span_lds", "runs") == (2, 8192, [[2, 1]])
    assert (2 - 1) * 1 + 8191 == cases.SCAN_SPAN_CAP
    # one symbol more than the staging area holds: k_hmm_scan<false>, 8 + 1 windows behind a non-zero stream base
    for pack, G22 in ((None, 1), ("0", 1), ("1", 2)):
        p = _plan("L8193", pack=pack)
        assert p["counts"] == [0, 8, 1] and p["launches"][22]["G"] == G22 and p["launches"][64]["G"] == 1
        assert all(not l["staged"] and l["span_lds"] == 0 and l["runs"] == [[8], [1]] for l in p["launches"].values())
    # the span rule, not waves x G x rounds, cuts the runs at every N
    for pack in cases.PACKS:
        p = _plan("L4000_H1000", pack=pack)
        assert p["counts"] == [0, 13, 6]
        for N in (5, 16, 64):
            assert pick(p, N, "cap", "span_lds", "runs") == (5, 8000, [[5, 5, 3], [5, 1]])
            assert cases.SCAN_WAVES * p["launches"][N]["G"] * 4 > 5
    # the rounds
    l = _plan("rounds_N1", rounds=64)["launches"][1]
    assert (l["G"], l["cap"], l["runs"], l["span_lds"]) == (64, 8156, [[8156, 808]], 8192) and 4 * 64 * 64 == 16384 > 8156
    l = _plan("rounds_N1", rounds=1)["launches"][1]
    assert (l["cap"], len(l["runs"][0]), l["runs"][0][-1]) == (256, 36, 4)
    assert _plan("rounds_N1", rounds=1000) == _plan("rounds_N1", rounds=64) and _plan("rounds_N1", rounds=0) == _plan("rounds_N1", rounds=1)
    p = _plan("rounds_N21_N64", rounds=64)
    assert pick(p, 21, "G", "cap", "runs") == (3, 768, [[768, 696]]) and pick(p, 64, "G", "cap", "runs") == (1, 256, [[256] * 5 + [184]])
    assert 768 // (cases.SCAN_WAVES * 3) == 64 == 256 // cases.SCAN_WAVES  # a wave takes 64 turns
    # a second launch of k_hmm_scan_wg, of 4 windows
    p = _plan("many_windows")
    assert p["W"] == (1 << 20) + 4 and p["big"] == [1] and p["wg_launches"] == 2 and p["W"] - cases.WG_WINDOWS_PER_LAUNCH == 4
    assert pick(p, 3, "G", "cap") == (21, 336) and len(p["launches"][3]["runs"][0]) == 3121
    # (the other figures of DESIGN.md 4.8.5's table, at the default pack width and rounds)
    assert _plan("L8192")["launches"][5]["lds"] == 18784 and pick(_plan("L8191"), 21, "G", "lds") == (3, 26968)
    assert [_plan("L8193")["launches"][N]["cap"] for N in (64, 22, 5)] == [16, 16, 192] and _plan("L8193", pack="1")["launches"][22]["cap"] == 32
    l = _plan("rounds_N1")["launches"][1]
    assert (l["cap"], len(l["runs"][0]), l["span_lds"]) == (1024, 9, 1060)
    assert [_plan("rounds_N21_N64")["launches"][N]["cap"] for N in (21, 64)] == [48, 16]
    # one window a stream at every huge hop, whatever the hop.  (At hop 8 the 150-symbol stream of huge_hop_short has seven
    # windows, not one: nine in all, a staged span of 148; windows 0, 1 and 8 of them are the three of the larger hops.)
    for hop in cases.HUGE_HOPS:
        for pack in cases.PACKS:
            p = _plan("huge_hop_long", hop, pack=pack)
            assert p["counts"] == [1, 1, 1] and all(l["span_lds"] == 0 and l["runs"] == [[1]] * 3 for l in p["launches"].values())
            p = _plan("huge_hop_short", hop, pack=pack)
            want = ([1, 7, 1], 148, [[1], [7], [1]]) if hop == 8 else ([1, 1, 1], 100, [[1]] * 3)
            assert p["counts"] == want[0] and all((l["span_lds"], l["runs"]) == want[1:] for l in p["launches"].values())


def _span_faults(formula):
    """(row, hop, pack, N) at which a launch is refused, or stages fewer symbols than its longest run covers"""
    bad = []
    for name, (Ns, _M, lens, L, hops) in cases.SCAN_SHAPES.items():
        for hop in hops:
            for pack in cases.PACKS:
                p = cases.scan_plan(Ns, lens, L, hop, pack=pack, formula=formula)
                true = cases.longest_true_span(p, L, hop)
                for N, l in p["launches"].items():
                    ok = 0 <= l["span_lds"] <= cases.SCAN_SPAN_CAP and not l["refused"]
                    if not ok or (l["span_lds"] != 0 and l["span_lds"] < true[N]):
                        bad.append((name, hop, pack, N))
                    if ok and l["span_lds"] == 0:  # read from global memory only where the longest run cannot be staged
                        assert true[N] > cases.SCAN_SPAN_CAP or formula == "parent", (name, hop, pack, N)
                    assert not ok or l["lds"] <= 49152
    return bad


def test_every_launch_stages_all_its_longest_run_covers():
    assert _span_faults("runs") == []
    # the record of the defect: (min(cap, W) - 1) hop + window wraps where W counts windows of several streams
    bad = _span_faults("parent")
    assert sorted(set((name, hop) for name, hop, _pack, _N in bad)) == [("huge_hop_long", 1 << 62), ("huge_hop_long", (1 << 63) - 1)]
    Ns, _M, lens, L, _hops = cases.SCAN_SHAPES["huge_hop_long"]
    l = cases.scan_plan(Ns, lens, L, 1 << 62, formula="parent")["launches"][64]
    assert l["span_lds"] == 8193 and l["refused"]                       # launch_scan returned without a launch
    l = cases.scan_plan(Ns, lens, L, (1 << 63) - 1, formula="parent")["launches"][64]
    assert l["span_lds"] == 8191 < L and l["staged"] and not l["refused"]  # staged, two symbols short of the window
    l = cases.scan_plan([5], [9000, 9000], 9000, (1 << 63) - 1, formula="parent")["launches"][5]
    assert l["span_lds"] == 8999 and l["refused"]
    assert not cases.scan_plan([5], [9000, 9000], 9000, (1 << 63) - 1)["launches"][5]["refused"]


# ---- the reference and the event cases, on the oracle alone ------------------------------------------------------------------
@pytest.fixture(scope="module")
def H():
    return oracle_lib.load_hmm()


def test_many_windows_has_all_16_pairs_and_costs_16_oracle_calls_a_model(H):
    models, streams, L, _hops = cases.scan_shape("many_windows")
    s = streams[0]
    assert (L, len(s)) == (2, (1 << 20) + 5) and s[:5].tolist() == [3, 3, 1, 0, 2] and s[-5:].tolist() == [0, 1, 3, 2, 0]
    pairs = lambda x: set(zip(x[:-1].tolist(), x[1:].tolist()))
    assert len(pairs(s[:5]) | pairs(s[-5:])) == 8 and len(pairs(s)) == 16
    ref = cases.shape_reference(H, "many_windows", 1)
    assert ref["oracle_calls"] == 16 * len(models) and ref["mant"].shape == (len(s) - 1, 2) and (ref["status"] == 0).all()
    for w in (0, 1, 2, 3, len(s) - 5, len(s) - 2, 77777):  # the expansion by keys puts each window's own result in its row
        for k, (pi, A, B) in enumerate(models):
            assert (ref["status"][w, k], ref["mant"][w, k], ref["exp2"][w, k]) == H.forward(pi, A, B, s[w:w + 2])


def test_the_rank_of_the_reference_is_the_top2_contract():
    st = np.array([[0, 0, 0], [0, 1, 0], [2, 1, 1], [0, 0, 0], [1, 0, 2]], np.int32)
    ex = np.array([[-3, -3, -4], [-9, 7, -9], [5, 6, 7], [-3, -2, -3], [0, -50, 0]], np.int64)
    ma = np.array([[.5, .5, .9], [.75, .9, .75], [.6, .7, .8], [.9, .5, .95], [.0, .5, .0]])
    best, second = cases.rank(st, ex, ma)
    # equal P: the later model first; P = 0 (any status but 0) below every P > 0, and equal among themselves
    assert best.tolist() == [1, 2, 2, 1, 1] and second.tolist() == [0, 0, 1, 2, 2]
    assert cases.rank(st[:, :1], ex[:, :1], ma[:, :1])[1].tolist() == [-1] * 5


@pytest.mark.parametrize("kind", cases.EVENT_KINDS)
@pytest.mark.parametrize("staged", [True, False])
def test_the_event_cases_put_each_status_at_both_ends_of_a_window(H, kind, staged):
    models, clean, dirty, L, hop = cases.events_case(kind) if staged else cases.unstaged_events_case(kind)
    at = cases.EVENT_AT if staged else cases.UNSTAGED_EVENT_AT
    assert all((s < cases.EVENT_M).all() for s in clean)
    assert kind == "outside" or all((s != cases.EVENT_DEAD).all() for s in clean)  # (no symbol but the planted ones is dead)
    assert [np.flatnonzero(d != c).tolist() for c, d in zip(clean, dirty)][1] == list(at)
    hit = cases.hits([len(s) for s in dirty], L, hop, 1, at)
    ts = {t for h in hit for t in h}
    assert {0, L - 1} <= ts and (ts == set(range(L)) if staged else ts == {0, 1, 2, 3, L - 1})
    ref = cases.reference(H, models, dirty, L, hop)
    want = np.array([cases.EVENT_STATUS[kind] if h else 0 for h in hit])
    assert (ref["status"] == want[:, None]).all() and (want == 0).sum() >= 4 and (want != 0).sum() >= 5
    assert np.isneginf(ref["log_prob"][want != 0]).all() and np.isfinite(ref["log_prob"][want == 0]).all()
    assert not ref["mant"][want != 0].any() and not ref["exp2"][want != 0].any()
    plan = cases.scan_plan([len(m[0]) for m in models], [len(s) for s in dirty], L, hop)
    assert all(l["staged"] == staged for l in plan["launches"].values()) and (plan["big"] == [3]) == staged
