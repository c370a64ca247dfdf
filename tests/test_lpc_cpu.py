"""CPU tests of the LPC front-end (`ecoz2 lpc`): the reference's per-frame helper ecoz2_lpca on its own fixture, the
exported symbols, the WAV reader, the frame count, the numpy restatement against ecoz2_lpca at every status, the CLI's
argument errors and the ISA of the NC = 37 kernel."""
import os
import re
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from tests import lpc_restatement as R
from tests import lpc_wavs
from tests.test_oracle import _load_lpca_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_ecoz2_lpca_on_reference_fixture(oracle):
    """signal_frame.inputs (frame 21 of a whale recording, P = 36): r, rc, a, pe bit-identical to the oracle and to the
    numpy restatement of lpca1 (src/lpc/lpca_rs.rs:28-75)."""
    x, p = _load_lpca_input()
    st, pe, r, rc, a = e.lpc.lpca(x, p)
    st_o, pe_o, r_o, rc_o, a_o = oracle.lpca(x, p)
    assert st == st_o == 0
    assert np.array_equal(_bits(r), _bits(r_o)) and np.array_equal(_bits(rc), _bits(rc_o))
    assert np.array_equal(_bits(a), _bits(a_o)) and _bits([pe]) == _bits([pe_o])
    r_n = R.autocorrelation(x[None, :], p)
    st_n, pe_n = R.levinson(r_n)
    assert st_n[0] == 0 and np.array_equal(_bits(r_n[0]), _bits(r)) and _bits(pe_n) == _bits([pe])


def test_ecoz2_lpca_status_codes():
    assert e.lpc.lpca(np.zeros(64), 8)[0] == 1
    with pytest.raises(e.Ecoz2Error, match="bad arguments"):
        e.lpc.lpca(np.ones(4), 4)  # p >= n
    assert e.lib.ecoz2_lpca(None, 4, 8, None, None, None, None) == -1


def test_reference_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ecoz2_vq.h")).read()
    assert re.search(r"int ecoz2_lpc_signals\(int prediction_order, int window_length_ms, int offset_length_ms, int minpc, "
                     r"float split,\s+const char \*const \*sgn_filenames, int num_signals, float mintrpt, int verbose\);", hdr)
    assert re.search(r"int ecoz2_lpca\(double \*x, int n, int p, double \*r, double \*rc, double \*a, double \*pe\);", hdr)
    syms = subprocess.run(["nm", "-D", "--defined-only", e.lib_path], capture_output=True, text=True, check=True).stdout
    for name in ("ecoz2_lpc_signals", "ecoz2_lpca", "e2vq_lpc_analyze", "e2vq_lpca_batch", "e2vq_wav_info",
                 "e2vq_lpc_frame_count"):
        assert re.search(r" T " + name + r"$", syms, re.M), name


@pytest.mark.skipif(e.lib.e2vq_device_count() > 0, reason="checks the behaviour without a HIP device")
def test_lpc_signals_without_device_fails_loudly(tmp_path):
    p = tmp_path / "A" / "x.wav"
    lpc_wavs.write_wav(p, np.arange(5000) % 100, 16000, 16)
    with pytest.raises(e.Ecoz2Error, match="no HIP device"):
        e.lpc.lpc_signals(36, 45, 15, 0, 0.0, [str(p)])
    with pytest.raises(e.Ecoz2Error, match="no HIP device"):
        e.lpc.analyze(np.arange(5000) % 100, 16000)


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_wav_reader_integer_pcm(tmp_path, bits):
    s = lpc_wavs.to_pcm(lpc_wavs.ar_source(bits, 8, 3000, 0.7), bits)
    s[:3] = [-(2 ** (bits - 1)), 2 ** (bits - 1) - 1, -1]
    p = tmp_path / f"s{bits}.wav"
    lpc_wavs.write_wav(p, s, 22050, bits)
    assert e.lpc.wav_info(p) == (22050, 3000, bits)
    got, sr = e.lpc.wav_read(p)
    assert sr == 22050 and np.array_equal(got, s)
    # WAVE_FORMAT_EXTENSIBLE with the PCM subformat reads the same
    q = tmp_path / f"x{bits}.wav"
    raw = open(p, "rb").read()
    data = raw[raw.index(b"data") + 8:]
    lpc_wavs.write_wav_raw(q, 0xFFFE, 1, 22050, bits, data, extensible_sub=1)
    assert np.array_equal(e.lpc.wav_read(q)[0], s)


def test_wav_reader_rejects_other_formats(tmp_path):
    cases = {
        "stereo.wav": (dict(fmt_code=1, channels=2, sample_rate=16000, bits=16, payload=b"\0" * 400), "2 channels"),
        "float.wav": (dict(fmt_code=3, channels=1, sample_rate=16000, bits=32, payload=b"\0" * 400), "IEEE float"),
        "float_ext.wav": (dict(fmt_code=0, channels=1, sample_rate=16000, bits=32, payload=b"\0" * 400,
                               extensible_sub=3), "IEEE float"),
        "u8.wav": (dict(fmt_code=1, channels=1, sample_rate=16000, bits=8, payload=b"\0" * 400), "8-bit"),
        "truncated.wav": (dict(fmt_code=1, channels=1, sample_rate=16000, bits=16, payload=b"\0" * 400,
                               declared_data=4000), "truncated"),
    }
    for name, (kw, what) in cases.items():
        p = tmp_path / name
        lpc_wavs.write_wav_raw(p, **kw)
        with pytest.raises(e.Ecoz2Error) as ei:
            e.lpc.wav_info(p)
        assert str(p) in str(ei.value) and what in str(ei.value), str(ei.value)
    (tmp_path / "junk.wav").write_bytes(b"not a wav file at all")
    with pytest.raises(e.Ecoz2Error, match="junk.wav: not a RIFF/WAVE file"):
        e.lpc.wav_info(tmp_path / "junk.wav")


def test_frame_count_edges():
    for sr in (16000, 22050, 32000, 44100):
        win, off, _ = R.geometry(10 ** 6, sr, 45, 15)
        for N in (win - 1, win, win + 1, win + off - 1, win + off, win + 7 * off - 1, 10 ** 6):
            assert e.lpc.frame_count(N, sr) == R.geometry(N, sr, 45, 15), (sr, N)
    assert e.lpc.frame_count(1440, 32000) == (1440, 480, 1)
    assert e.lpc.frame_count(1440 + 480 - 1, 32000) == (1440, 480, 1)
    assert e.lpc.frame_count(1439, 32000)[2] == -1
    assert e.lpc.frame_count(100000, 22050)[:2] == (992, 330)  # 45 * 22050 / 1000 = 992.25 truncates
    with pytest.raises(e.Ecoz2Error, match="zero samples"):
        e.lpc.frame_count(100000, 50, 45, 15)


def test_restatement_matches_lpca_frame_by_frame():
    """The numpy restatement (vectorised across frames) equals ecoz2_lpca run frame by frame, silent stretch included."""
    s = lpc_wavs.to_pcm(lpc_wavs.ar_source(3, 12, 16000, 0.5), 16)
    s[4000:9000] = 7  # a constant stretch: zero after mean removal -> status 1
    frames, status = R.analyze(s, 16000, P=12)
    w = R.windowed_frames(s, 16000, 45, 15)
    assert (status == 1).sum() > 0 and (status == 0).sum() > 0
    for t in range(len(status)):
        st, pe, r, _rc, _a = e.lpc.lpca(w[t], 12)
        assert st == status[t]
        if st == 0:
            assert np.array_equal(_bits(r / pe), _bits(frames[t]))


# ---- rows that reach every Levinson status through a real autocorrelation (shared with test_gpu_lpc_shapes) --------------
LANE = (12, 16, 20, 24, 28, 32, 36, 40)  # orders with a lane-per-frame instantiation (E2VQ_LPC_NC_LIST)
GENERIC = (1, 2, 13, 41, 79, 80)  # block-per-frame path: the smallest orders, just off a lane order, the largest
# cos(2 pi f k) times 1e-161 and 3e-162: the squares land in the subnormal range, where pe * (1 - akk^2) rounds to <= 0
# (status 2) for some rows and not for others; times 1e-162 every square underflows to zero (r[0] == 0: status 1).
# Two orders' worth of exceptions, picked on the CPU with the restatement: at P >= 79 no row scaled by 1e-161 or less
# keeps status 0 at most frame lengths, and at P = 1, n = 2 no row scaled by 3e-162 or more reaches status 2.
def subnormal_scales(P):
    return ((3e-161, 1e-161) if P >= 79 else (3e-162, 2e-162) if P == 1 else (1e-161, 3e-162)) + (1e-162,)


def frame_lengths(NC):
    """Around each phase of the lane kernel's autocorrelation: first NC samples only, no main loop, an empty tail."""
    return (NC, NC + 1, 2 * NC - 1, 2 * NC, 2 * NC + 1, 2 * NC + 3, 3 * NC, 3 * NC + 7)


def subnormal_rows(P, n):
    f = np.linspace(0.001, 0.45, 200)
    x = np.cos(2 * np.pi * f[:, None] * np.arange(n)[None, :])
    return np.concatenate([x * sc for sc in subnormal_scales(P)])


def lpca_rows(P, n):
    """Windowed frames (rows, n): seeded normal rows, two AR rows, a zero row, a row that is zero except for its last
    sample, and the subnormal-scale rows."""
    rng = np.random.default_rng(1000 * P + n)
    last = np.zeros((1, n))
    last[0, -1] = 0.75
    ar = [lpc_wavs.ar_source(s, 10, n, 0.6)[None, :] for s in (21, 22)]
    return np.concatenate([rng.standard_normal((8, n)), *ar, np.zeros((1, n)), last, subnormal_rows(P, n)])


@pytest.mark.parametrize("P", LANE + GENERIC)
def test_restatement_lpca_matches_host_lpca_at_every_status(P):
    """R.lpca (frozen rows: what lpca1 leaves in pe, rc and a when it stops) against host ecoz2_lpca, row by row on the
    bits, on the rows the GPU test uses at this order.  The subnormal-scale rows alone give statuses 0, 1 and 2 at every
    frame length (asserted here on the restatement, before the host is asked).  Status 1: the host returns before it
    writes rc and a, so only status, pe and r are compared.  These rows give no NaN or infinity in rc or a (pe <= 0 ends
    the recursion first); the comparison still goes by NaN position.  Signal mode cannot be steered into status 2:
    integer sinusoids (16- and 32-bit, P up to 80) and unscaled cosines never gave it, so no test tries."""
    for n in frame_lengths(P + 1):
        x = lpca_rows(P, n)
        st, pe, r, rc, a = R.lpca(x, P)
        assert set(st[-600:]) == {0, 1, 2}, (P, n)
        assert st[10] == 1 and st[11] == 0 and (st[:10] == 0).all(), (P, n)
        for t in range(len(x)):
            st_h, pe_h, r_h, rc_h, a_h = e.lpc.lpca(x[t], P)
            assert st_h == st[t] and _bits([pe_h]) == _bits(pe[t:t + 1]), (P, n, t)
            assert np.array_equal(_bits(r_h), _bits(r[t])), (P, n, t)
            if st_h != 1:
                for got, ref in ((rc_h, rc[t]), (a_h, a[t])):
                    nan = np.isnan(ref)
                    assert np.array_equal(np.isnan(got), nan), (P, n, t)
                    assert np.array_equal(_bits(got[~nan]), _bits(ref[~nan])), (P, n, t)


def test_restatement_lpca_agrees_with_levinson():
    """On rows that do not fail, the frozen restatement and the one `analyze` uses are the same numbers."""
    x = lpca_rows(12, 29)
    st, pe, r, _rc, _a = R.lpca(x, 12)
    st_l, pe_l = R.levinson(r)
    assert np.array_equal(st, st_l) and np.array_equal(_bits(pe[st == 0]), _bits(pe_l[st == 0]))


def _cli(*args, cwd=None):
    return subprocess.run([EXE, "lpc", *args], capture_output=True, text=True, cwd=cwd, timeout=60)


def test_cli_argument_errors(tmp_path):
    r = _cli()
    assert r.returncode == 2 and "--signals" in r.stderr
    for flag in ("--zrs", "--zrsp"):
        r = _cli(flag, "--signals", "x.wav")
        assert r.returncode == 2 and "CBOR" in r.stderr and flag in r.stderr
    r = _cli("-P", "81", "--signals", "x.wav")
    assert r.returncode == 2 and "out of range" in r.stderr
    r = _cli("-O", "0", "--signals", "x.wav")
    assert r.returncode == 2
    r = _cli("-P", "abc", "--signals", "x.wav")
    assert r.returncode == 2 and "invalid value" in r.stderr
    r = _cli("--bogus", "--signals", "x.wav")
    assert r.returncode == 2 and "usage" in r.stderr
    r = _cli("--signals", "missing.csv", cwd=tmp_path)
    assert r.returncode == 0 and "cannot open" in r.stdout


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_isa_lane_kernel_nc37_no_scratch_no_spill(tmp_path):
    out = tmp_path / "lpc.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-x", "hip",
                    "--cuda-device-only", "-S", "-DE2VQ_LPC_NC_LIST(X)=X(37)", "-o", str(out),
                    os.path.join(ROOT, "ecoz2rs_amd", "csrc", "lpc_device.hip")], check=True, timeout=900,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = out.read_text()
    metas = [(m.group(1), m.group(2)) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S)
             if "k_lpc_lane" in m.group(1)]
    assert len(metas) == 2, [n for n, _ in metas]  # signal and windowed-frame instantiations at NC = 37
    for name, meta in metas:
        assert "ILi37E" in name
        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", meta).group(1))  # noqa: E731
        assert g("private_segment_fixed_size") == 0, name
        assert g("vgpr_spill_count") == 0, name
        assert g("vgpr_count") <= 512, name
