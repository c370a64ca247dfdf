"""`vq classify` on the GPU against the oracle (ecoz2_vq_classify in vq_entry.cpp; e2vq_set_codebook + e2vq_quantize_device
switching codebooks inside one session in vq_host.cpp): every printed score, the class table, the refusals and the CLI
compared with tests/vq_classify_cases.py -- stdout as text equal byte for byte, symbols with array_equal, doubles on their
bits; no tolerance.  The inputs reach every route of e2vq_quantize_device (plain, row-major, blockified, generic, prefiltered
fused and unfused with its FP64 fallback), the reuse, rebuild and regrowth of the cached codebook image across switches, and
every branch of the unit plan (batch, exact fit, flush, cut, empty file) at three chunk settings;
tests/test_vq_classify_cases_cpu.py holds those inputs against the oracle alone."""
import os
import re
import subprocess

import numpy as np
import pytest

import ecoz2rs_amd as e
from tests import vq_classify_cases as vc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "ecoz2rs_amd", "csrc", "ecoz2")
_written = {}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("ECOZ2_VQ_QUANTIZE_CHUNK", "ECOZ2_VQ_QUANTIZE_UNFUSED", "ECOZ2_VQ_PREFILTER", "ECOZ2_VQ_PREFILTER_MIN_M"):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture
def corpus(tmp_path_factory):
    """name -> (case, its root, codebook paths, predictor paths): each case written once per run"""
    def get(name):
        if name not in _written:
            root = tmp_path_factory.mktemp("vqc_" + name)
            _written[name] = (vc.case(name), root) + vc.case(name).write(root)
        return _written[name]
    return get


def _settings(monkeypatch, chunk, unfused):
    if chunk is not None:
        monkeypatch.setenv("ECOZ2_VQ_QUANTIZE_CHUNK", str(chunk))
    if unfused:
        monkeypatch.setenv("ECOZ2_VQ_QUANTIZE_UNFUSED", "1")


def _classify(cbs, prds, ranked, capfd):
    capfd.readouterr()
    e.vq_classify(cbs, prds, show_ranked=ranked)
    return capfd.readouterr().out


def _first_difference(got, want):
    for n, (a, b) in enumerate(zip(got.splitlines(), want.splitlines())):
        if a != b:
            return "line %d:\n got  %s\n want %s" % (n, a, b)
    return "%d lines against %d" % (len(got.splitlines()), len(want.splitlines()))


# ---- 1. the scores of every pair -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("unfused", [False, True], ids=["fused", "unfused"])
@pytest.mark.parametrize("chunk", vc.CHUNKS, ids=lambda c: "chunk_%s" % c)
def test_every_score_at_every_size(corpus, monkeypatch, capfd, chunk, unfused):
    """P = 36, the eleven codebooks of M_ORDER_36 against the thirteen files of LENGTHS_36, every file under a class name no
    codebook has: all of them are reported with the score of every codebook"""
    c, _root, cbs, prds = corpus("sizes36")
    _settings(monkeypatch, chunk, unfused)
    got, want = _classify(cbs, prds, True, capfd), c.report(prds, True)
    assert want.count("ranked:") == sum(T > 0 for T in c.Ts) == 11 and len(cbs) == 11
    assert got == want, _first_difference(got, want)


# ---- 2. the table and the ties -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranked", [False, True], ids=["table", "ranked"])
@pytest.mark.parametrize("chunk", [None, 1024], ids=lambda c: "chunk_%s" % c)
def test_table_and_ties(corpus, monkeypatch, capfd, chunk, ranked):
    """true and wrong labels, two codebooks of identical reflections (the earlier one wins, the ranking keeps their order),
    an empty file, a class of empty files only"""
    c, _root, cbs, prds = corpus("table")
    _settings(monkeypatch, chunk, False)
    got, want = _classify(cbs, prds, ranked, capfd), c.report(prds, ranked)
    assert got == want, _first_difference(got, want)
    assert ("Bdup(" in got) == ranked and "\nE " not in got and "TOTAL                           7        3   42.86%" in got


# ---- 3. the other orders -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,unfused", [(20, False), (20, True), (40, False), (40, True), (48, False), (100, False)])
@pytest.mark.parametrize("chunk", vc.CHUNKS, ids=lambda c: "chunk_%s" % c)
def test_every_score_at_other_orders(corpus, monkeypatch, capfd, chunk, P, unfused):
    """P = 20 and 40 (prefilter orders, fused and unfused; 40 runs seven waves), 48 (wide MFMA: blockified, never
    prefiltered), 100 (generic): M = 256, 8, 300 against files of 1, 65, 700 and 1025 frames"""
    c, _root, cbs, prds = corpus("sizes%d" % P)
    _settings(monkeypatch, chunk, unfused)
    got, want = _classify(cbs, prds, True, capfd), c.report(prds, True)
    assert want.count("ranked:") == 4 and len(cbs) == 3
    assert got == want, _first_difference(got, want)


# ---- 4. switching in one session, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("P,unfused", [(36, False), (36, True), (40, False), (40, True), (48, False)])
def test_switching_codebooks_in_one_session(monkeypatch, P, unfused):
    """one session without frames, as classify makes it: set_codebook + quantize over SWITCH_36 (SWITCH_48: sizes to 2048) with
    1, 65, 3000, 700, ... frames -- the same M with other contents and back, plain <-> prefiltered, across 2048 and back,
    8224 -> 64 -> 256; after every step the symbols, the bits of dmin and the average distortion are the oracle's"""
    _settings(monkeypatch, None, unfused)
    with e.VqSession(P) as s:
        for q, (name, refl, frames, sym_o, dmin_o) in enumerate(vc.switch_steps(P)):
            s.set_codebook(refl)
            sym, dmin = s.quantize(frames)
            assert np.array_equal(sym, sym_o), (q, name, len(frames))
            assert np.array_equal(dmin.view(np.uint64), dmin_o.view(np.uint64)), (q, name, len(frames))
            # (a second quantize under the same codebook: the cached image is reused)
            avg = s.avg_distortion(frames)
            assert np.float64(avg).view(np.uint64) == np.float64(vc.score(dmin_o)).view(np.uint64), (q, name, len(frames))


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
def _refused(cbs, prds, capfd, message):
    capfd.readouterr()
    with pytest.raises(e.Ecoz2Error, match=message):
        e.vq_classify(cbs, prds, show_ranked=True)
    assert capfd.readouterr().out == ""


def test_refusals(corpus, tmp_path, monkeypatch, capfd):
    c, _root, cbs, prds = corpus("table")
    other = vc.sizes_case(20)
    cb20 = str(tmp_path / "p20.cbook")
    e.formats.write_cbook(cb20, "B", other.cbs[1][1])
    prd20 = str(tmp_path / "p20.prd")
    e.formats.write_prd(prd20, "B", other.files[1][3])
    _refused(cbs + [cb20], prds, capfd, re.escape(cb20) + ": prediction order differs from the first codebook")
    _refused(cbs, prds + [prd20], capfd, re.escape(prd20) + ": prediction order 20 differs from the codebooks' 36")
    _refused([], prds, capfd, "ecoz2_vq_classify: bad arguments")
    # a NaN in the last frame of the last piece of a cut file, behind files that have been swept already
    frames = c.files[9][3].copy()
    assert len(frames) == 1500 and vc.units(c.Ts[:9] + [1500], 1024)[-1] == [(9, 1024, 476, 0)]
    frames[-1, 36] = np.nan
    bad = str(tmp_path / "late_nan.prd")
    e.formats.write_prd(bad, "B", frames)
    monkeypatch.setenv("ECOZ2_VQ_QUANTIZE_CHUNK", "1024")
    _refused(cbs, prds[:9] + [bad], capfd, re.escape(bad) + ": contains NaN or infinite values")
    frames[-1, 36] = np.inf
    e.formats.write_prd(bad, "B", frames)
    _refused(cbs, prds[:9] + [bad], capfd, re.escape(bad) + ": contains NaN or infinite values")


# ---- 6. the CLI ----------------------------------------------------------------------------------------------------------
def test_cli(corpus):
    """`ecoz2 vq classify -r --codebooks <dir> --tt TEST --predictors tt.csv` on the table case: the codebooks in sorted
    path order (A, B, Bdup, C: B takes the tie now), the TEST rows of the list in its order"""
    c, root, _cbs, _prds = corpus("table")
    rows = ["tt,class,selection", "TRAIN,A,00000", "TRAIN,Z,99999"]
    rows += ["TEST,%s,%s" % (d, sel) for d, sel, _label, _f in c.files] + ["TRAIN,B,00001"]
    (root / "tt.csv").write_text("\n".join(rows) + "\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("ECOZ2_VQ_")}
    r = subprocess.run([CLI, "vq", "classify", "-r", "--codebooks", "data/codebooks", "--tt", "TEST", "--predictors", "tt.csv"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr, r.stderr
    order = sorted(range(len(c.cbs)), key=lambda i: c.cbs[i][0])
    assert [c.cbs[i][0] for i in order] == ["A", "B", "Bdup", "C"]
    paths = ["data/predictors/%s/%s.prd" % (d, sel) for d, sel, _label, _f in c.files]
    want = ("number of codebooks: 4  number of predictors: %d\nshow_ranked = true\n" % len(paths)
            + c.report(paths, True, cb_order=order))
    assert r.stdout == want, _first_difference(r.stdout, want)
    assert "data/predictors/Bdup/00000.prd: 'Bdup' classified as 'B'; ranked: B(" in r.stdout
