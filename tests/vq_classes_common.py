"""Helpers of the `vq learn --all-classes` GPU tests (test_gpu_vq_learn_classes.py, test_gpu_vq_learn_classes_shapes.py):
class data, per-class session ladders, bitwise comparison of ladders, .prd corpora and the single-class file loop."""
import numpy as np

import ecoz2rs_amd as e
from ecoz2rs_amd import vq
from ecoz2rs_amd._lib import LEARN_CALLBACK

EPS = 0.05


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _class_frames(P, sizes, seed=7):
    """class k: prototype frames (kind 0) for even k, corpus-shaped continuum frames (kind 1) for odd k"""
    out = []
    for k, T in enumerate(sizes):
        if k % 2 == 0:
            out.append(e.synth.synth_frames(seed + k, 4, P, 1000 * k, T))
        else:
            out.append(e.synth.synth_frames_kind(seed + k, 1, 4, 0.05, P, 1000 * k, T))
    return out


def _session_ladder(frames, P, max_M):
    with e.VqSession(P, device=0) as s:
        s.set_frames(frames)
        s.prepare()
        s.init_codebook()
        levels = s.learn(EPS, max_M)
        return s.get_codebook(), levels


def _same_levels(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x.M, x.passes, x.empty_cells, x.failed_cells) == (y.M, y.passes, y.empty_cells, y.failed_cells)
        assert _bits([x.DD, x.avg_distortion, x.sigma, x.inertia]).tolist() == _bits([y.DD, y.avg_distortion, y.sigma,
                                                                                        y.inertia]).tolist()


def _prd_corpus(root, P, sizes, seed=5):
    """one class per size, each split over up to three files, the list interleaving the classes; class names out of
    byte order of creation"""
    frames = _class_frames(P, sizes, seed)
    rng = np.random.default_rng(seed)
    per_class = {}
    for k, f in enumerate(frames):
        name = f"V{(k * 5) % len(sizes):02d}"
        cuts = sorted(set(rng.integers(1, len(f), 2).tolist())) if len(f) > 2 else []
        files = []
        for q, part in enumerate(np.split(f, cuts)):
            p = root / "data" / "predictors" / name / f"{q:05d}.prd"
            p.parent.mkdir(parents=True, exist_ok=True)
            e.formats.write_prd(str(p), name, part)
            files.append(str(p))
        per_class[name] = files
    order = []
    while any(per_class.values()):
        for name in list(per_class):
            if per_class[name]:
                order.append(per_class[name].pop(0))
    return order


def _read_tree(d):
    return {str(p.relative_to(d)): p.read_bytes() for p in sorted(d.rglob("*")) if p.is_file()}


def _single_loop(files, P, out, monkeypatch, capfd):
    monkeypatch.setenv("ECOZ2_VQ_OUT_ROOT", str(out))
    by_class = {}
    for f in files:
        by_class.setdefault(e.formats.read_prd(f)[0], []).append(f)
    seen = []
    cb = LEARN_CALLBACK(lambda _t, m, a, s, i: seen.append((m, a, s, i)))
    capfd.readouterr()
    for name in sorted(by_class, key=lambda s: s.encode()):
        fs, _keep = vq._to_vec_of_ptr_const_c_char(by_class[name])
        assert e.lib.ecoz2_vq_learn(P, EPS, name.encode(), fs, len(by_class[name]), None, cb) == 0, e.lib.e2vq_last_error()
    return _read_tree(out), seen, capfd.readouterr().out, len(by_class)


def _batched(files, P, out, monkeypatch, capfd):
    monkeypatch.setenv("ECOZ2_VQ_OUT_ROOT", str(out))
    seen = []
    capfd.readouterr()
    vq.vq_learn_classes(P, EPS, files, callback=lambda *a: seen.append(a))
    return _read_tree(out), seen, capfd.readouterr().out
