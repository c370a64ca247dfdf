"""Synthetic WAV corpora for the LPC tests (TEST INFRASTRUCTURE): seeded AR sources written with the stdlib `wave`."""
import functools
import os
import struct
import wave

import numpy as np


@functools.lru_cache(maxsize=64)
def _ar(seed, order, n, amplitude):
    return ar_source_uncached(seed, order, n, amplitude)


def ar_source(seed, order, n, amplitude):
    """Cached: the array is the caller's to change."""
    return _ar(seed, order, n, amplitude).copy()


def ar_source_uncached(seed, order, n, amplitude):
    """A stable AR(order) process (random reflection coefficients |k| < 0.85, step-up to the predictor), n samples."""
    rng = np.random.default_rng(seed)
    k = rng.uniform(-0.85, 0.85, order)
    a = np.zeros(order + 1)
    a[0] = 1.0
    for m in range(1, order + 1):
        prev = a.copy()
        for i in range(1, m):
            a[i] = prev[i] + k[m - 1] * prev[m - i]
        a[m] = k[m - 1]
    e = rng.standard_normal(n + 200)
    y = np.zeros(n + 200)
    for t in range(n + 200):
        acc = e[t]
        for j in range(1, min(order, t) + 1):
            acc -= a[j] * y[t - j]
        y[t] = acc
    y = y[200:]
    return y / (np.abs(y).max() + 1e-12) * amplitude


def to_pcm(y, bits):
    full = 2 ** (bits - 1) - 1
    return np.clip(np.round(y * full), -full - 1, full).astype(np.int64)


def write_wav(path, samples, sample_rate, bits):
    d = os.path.dirname(str(path))
    if d:
        os.makedirs(d, exist_ok=True)
    s = np.asarray(samples, dtype=np.int64)
    if bits == 16:
        raw = s.astype("<i2").tobytes()
    elif bits == 32:
        raw = s.astype("<i4").tobytes()
    else:
        b = s.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]
        raw = b.tobytes()
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(bits // 8)
        w.setframerate(sample_rate)
        w.writeframes(raw)


def write_wav_raw(path, fmt_code, channels, sample_rate, bits, payload, extensible_sub=None, declared_data=None):
    """A RIFF/WAVE file built by hand (formats `wave` does not write: float, WAVE_FORMAT_EXTENSIBLE, truncated)."""
    block = channels * bits // 8
    if extensible_sub is None:
        fmt = struct.pack("<HHIIHH", fmt_code, channels, sample_rate, sample_rate * block, block, bits)
    else:
        guid = struct.pack("<H", extensible_sub) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, channels, sample_rate, sample_rate * block, block, bits, 22, bits, 4) + guid
    n = len(payload) if declared_data is None else declared_data
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", n) + payload
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
