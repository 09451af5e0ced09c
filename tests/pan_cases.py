"""Crafted streams for the panorama tests (tests/test_pan.py, tests/test_gpu_pan.py): seeded noise with two tones
60 dB apart for every kind, single tones, impulses, and the chunkings of a stream."""
from functools import lru_cache

import numpy as np

from pyft8_amd import kinds as K
from pyft8_amd import pan

KINDS = list(pan.KINDS)
KIND_IDS = {K.REAL_I16: "real_i16", K.REAL_F32: "real_f32", K.IQ_I16: "iq_i16", K.IQ_F32: "iq_f32", K.WIDE_REAL_I16: "wide_real_i16",
            K.WIDE_IQ_I16: "wide_iq_i16", K.WIDE_IQ_U8: "wide_iq_u8", K.WIDE_IQ_I8: "wide_iq_i8"}
INT_KINDS = [k for k in KINDS if K.is_integer(k)]
SIZES = [256, 2048, 8192]
AVGS = [1, 3, 37]


def store(v, kind):
    """complex (IQ) or real float64 values on the int16 scale -> packed samples of the kind, rounded and clipped"""
    dt = np.dtype(K.DTYPE[kind])
    a = np.stack([v.real, v.imag], axis=1) if K.is_iq(kind) else np.asarray(v.real if np.iscomplexobj(v) else v)
    if dt.kind == "f":
        return np.ascontiguousarray(a, np.float32)
    if dt == np.uint8:
        a = a / 256.0 + 127.5
    elif dt == np.int8:
        a = a / 256.0
    info = np.iinfo(dt)
    return np.ascontiguousarray(np.clip(np.rint(a), info.min, info.max).astype(dt))


def tone(kind, n, cycles_per_sample, amp=20000.0, phase=0.3):
    """one tone: an exponential for an IQ kind, a cosine for a real one"""
    ph = 2.0 * np.pi * cycles_per_sample * np.arange(n) + phase
    return amp * (np.exp(1j * ph) if K.is_iq(kind) else np.cos(ph))


@lru_cache(maxsize=None)
def noisy(kind, n, seed=11):
    """seeded noise plus two tones 60 dB apart (amplitudes 16000 and 16): the weak one is above the noise of a window only for the
    16-bit and float kinds, which is the point -- the 8-bit kinds bury it in their rounding"""
    rng = np.random.default_rng(seed + 1000 * kind)
    noise = 600.0 * (rng.standard_normal(n) + (1j * rng.standard_normal(n) if K.is_iq(kind) else 0.0))
    v = noise + tone(kind, n, 0.1371, 16000.0) + tone(kind, n, 0.3127, 16.0, 1.1)
    a = store(v, kind)
    a.setflags(write=False)
    return a


def accuracy_n(n_fft, n_avg):
    return (2 * n_avg + 1) * n_fft + 37


def chunkings(n, N, A, max_push, seed=5):
    """name -> the lengths of the pushes of a stream of n samples"""
    def rest(head):
        head = [c for c in head if c > 0]
        assert sum(head) <= n and max(head, default=0) <= max_push
        tail = n - sum(head)
        return head + [max_push] * (tail // max_push) + ([tail % max_push] if tail % max_push else [])
    rng = np.random.default_rng(seed)
    rnd = []
    while sum(rnd) < n:
        rnd.append(int(min(rng.integers(1, max_push + 1), n - sum(rnd))))
    out = {"edges": rest([1, N - 1, N, N + 1, A * N - 1, A * N + 1]),
           "single_samples": rest([N - 3] + [1] * 6 + [A * N - N - 6] * (A > 1) + [1] * 6),
           "random": rnd}
    if n <= max_push:
        out["at_once"] = [n]
    return out


def cut(x, lengths):
    out, at = [], 0
    for c in lengths:
        out.append(x[at:at + c])
        at += c
    assert at == len(x)
    return out
