"""Wide pre-decimator: ONE stream at 240 kHz .. 129.6 MHz -- real int16, IQ int16, IQ uint8 (RTL-SDR), IQ int8
(HackRF) -- in front of the down-converter of ddc.py.

The GPU stage is ft8rx_ddc_wide* (Handle.ddc_wide, Handle.ddc_wide_stream_*, Receiver.decode_stream).  Here: the kinds, the plan of a
rate and the taps of the pre-filter (both from the library, the single source), the frequency words, and the float64 twins of the
definition.  The twins make only the intermediate samples that are asked for, by direct dot products, so that the 64.8 MHz cases need
neither the whole stream at once nor a long FFT."""
import sys

import numpy as np

from . import _lib
from . import ddc as _ddc
from . import kinds as _k

REAL_I16, IQ_I16, IQ_U8, IQ_I8 = _k.WIDE_REAL_I16, _k.WIDE_IQ_I16, _k.WIDE_IQ_U8, _k.WIDE_IQ_I8      # include/ft8rx.h FT8RX_WIDE_*
KINDS, KIND_NAMES, _DTYPE = _k.view((REAL_I16, IQ_I16, IQ_U8, IQ_I8))
NSAMP = _lib.NSAMP
TILE = 1008


def _kind(kind):
    if kind not in KINDS:
        raise _lib.Ft8rxError(f"kind {kind} is not one of REAL_I16, IQ_I16, IQ_U8, IQ_I8 (ddc_wide)")
    return kind


def is_iq(kind):
    return _k.is_iq(_kind(kind))


def kind_of(samples, iq):
    """The kind of an array by its dtype: uint8 / int8 / int16 (I, Q) pairs [n, 2] with iq, int16 [n] without.  Float or complex input
    is refused, naming the dtype: at these rates the sources deliver integers."""
    a = np.asarray(samples)
    if a.dtype == np.int16:
        return IQ_I16 if iq else REAL_I16
    if iq and a.dtype == np.uint8:
        return IQ_U8
    if iq and a.dtype == np.int8:
        return IQ_I8
    raise _lib.Ft8rxError(f"samples: dtype {a.dtype} is not taken at a wide rate (iq: uint8, int8 or int16 pairs; real: int16)")


def accepts(rate):
    """True for a rate the pre-decimator takes (a multiple of 48000 in [240000, 129600000] with R0 <= 1350)."""
    try:
        return _lib.lib().ft8rx_ddc_wide_plan(int(rate), None, None) == 0
    except (TypeError, ValueError, OverflowError):
        return False


def plan(rate):
    """(rate_mid, R0) of a rate: the largest of 192000, 96000, 48000 that divides it with R0 = rate / rate_mid >= 2; anything else is
    refused (ft8rx_ddc_wide_plan)."""
    mid, r0 = np.zeros(1, np.int32), np.zeros(1, np.int32)
    if not isinstance(rate, (int, np.integer)) or not -2 ** 31 <= rate < 2 ** 31 or \
            _lib.lib().ft8rx_ddc_wide_plan(int(rate), mid.ctypes.data, r0.ctypes.data) != 0:
        raise _lib.Ft8rxError(f"rate {rate} is not a multiple of 48000 in [240000, 129600000] with rate / rate_mid <= 1350")
    return int(mid[0]), int(r0[0])


def taps(rate):
    """float32 taps of the pre-filter h0 at `rate`, as the kernel uses them (ft8rx_ddc_wide_taps)."""
    plan(rate)
    buf = np.zeros(8448, np.float32)
    n = _lib.lib().ft8rx_ddc_wide_taps(int(rate), buf.ctypes.data, len(buf))
    if n < 0:
        raise _lib.Ft8rxError(f"ddc_wide.taps: no filter for rate {rate}")
    return buf[:n].copy()


def _words(rate, rate_mid, f_dial_hz):
    """frequency_words behind the plan (this module's and ddc_rat's)"""
    w0 = int(np.rint((float(f_dial_hz) + 3000.0) / float(rate) * 4294967296.0)) % (1 << 32)
    f0 = w0 * float(rate) / 4294967296.0
    if f0 >= 0.5 * rate:
        f0 -= rate
    d = float(f_dial_hz) - f0
    d -= rate * np.rint(d / rate)
    f = f0 + _ddc.frequency_word(rate_mid, d)[1]
    f = f - rate if f >= 0.5 * rate else f + rate if f < -0.5 * rate else f
    return w0, f0, float(d), float(f)


def frequency_words(rate, f_dial_hz):
    """(w0, f0, dial_mid, f_mixed_hz) of a dial `f_dial_hz` from the stream's centre: the pre-stage's 32-bit frequency word, the
    frequency it really mixes (in [-rate/2, rate/2)), the dial left for the down-converter behind it (f_dial - f0, about -3000 Hz) and
    the dial the whole chain really mixes."""
    return _words(rate, plan(rate)[0], f_dial_hz)


def pack(samples, kind):
    """One stream's samples as the C-contiguous array ft8rx_ddc_wide takes for `kind` -> (array, n): real int16 [n]; IQ kinds (I, Q)
    pairs [n, 2] of int16, uint8 or int8."""
    return _k.pack_stream(samples, _kind(kind), "samples: {name} is ONE stream, {form}, got shape {shape}",
                          "samples: {name} needs integers in the {dtype} range, got dtype {got}")


def sample_values(x, kind):
    """One stream's samples as float64 [n] (real) or complex128 [n] (IQ) on the int16 scale: uint8 u -> 256 (u - 127.5), int8 s -> 256 s.
    (The twins also take values that are on that scale already: float [n] for the real kind, complex [n] for the IQ kinds.)"""
    a = np.asarray(x)
    if a.ndim == 1 and a.dtype.kind == ("c" if is_iq(kind) else "f"):
        return a.astype(np.complex128 if is_iq(kind) else np.float64)
    return _k.values(pack(x, kind)[0], kind)


def _phasor(p):
    """e^{-2 pi i p / 2^32} for integer phases p (uint64 below 2^32)"""
    return np.exp(-2j * np.pi * (p.astype(np.float64) / 4294967296.0))


def _mid(xv, iq, rate, f_dial_hz, k_lo, k_hi, n_origin):
    """reference_mid on sample values (float64 real or complex128)"""
    _, R0 = plan(rate)
    if not -0.5 * rate <= f_dial_hz < 0.5 * rate:
        raise _lib.Ft8rxError(f"f_dial_hz {f_dial_hz} outside [-rate / 2, rate / 2)")
    k_lo, k_hi, n_origin = int(k_lo), int(k_hi), int(n_origin)
    if k_hi <= k_lo or n_origin < 0:
        raise _lib.Ft8rxError(f"intermediate samples [{k_lo}, {k_hi}) / n_origin {n_origin}: need k_lo < k_hi and n_origin >= 0")
    h0 = taps(rate).astype(np.float64)
    N0, C0 = len(h0), (len(h0) - 1) // 2
    w0 = frequency_words(rate, f_dial_hz)[0]
    W = h0 * _phasor((np.arange(N0, dtype=np.uint64) * np.uint64(w0)) & np.uint64(0xFFFFFFFF))
    n_a, n_b = k_lo * R0 - C0, (k_hi - 1) * R0 + C0 + 1                     # the inputs under the outputs asked for
    xs = np.zeros(n_b - n_a, xv.dtype)
    lo, hi = max(n_a, n_origin), min(n_b, n_origin + len(xv))
    if hi > lo:
        xs[lo - n_a:hi - n_a] = xv[lo - n_origin:hi - n_origin]
    it = xs.strides[0]
    win = np.lib.stride_tricks.as_strided(xs, shape=(k_hi - k_lo, N0), strides=(R0 * it, it), writeable=False)
    v = np.empty(k_hi - k_lo, np.complex128)
    rows = max(1, (1 << 21) // N0)
    for a in range(0, len(v), rows):
        v[a:a + rows] = win[a:a + rows] @ W
    first = (np.arange(k_lo, k_hi, dtype=np.int64) * R0 - C0) % (1 << 32)   # (k R0 - C0) mod 2^32: the phase of the output's first input
    rot = _phasor((first.astype(np.uint64) * np.uint64(w0)) & np.uint64(0xFFFFFFFF))
    return (1.0 if iq else 2.0) * rot * v


def reference_mid(x, kind, rate, f_dial_hz, k_lo, k_hi, n_origin=0):
    """The float64 twin of the pre-stage alone: intermediate samples v[k], k_lo <= k < k_hi (absolute), of one channel -> complex128.
    x[0] has the absolute index n_origin; the stream is zero before it and after its end.  Library taps, exact integer phases."""
    return _mid(sample_values(x, kind), is_iq(kind), rate, f_dial_hz, k_lo, k_hi, n_origin)


def mid_count(n_samples, rate):
    """Intermediate samples of a one-shot call on n_samples inputs (csrc/ddc_wide_ring.hpp: mid_count)"""
    rate_mid, R0 = plan(rate)
    if n_samples < 1:
        return 1
    return min((n_samples - 1 + (len(taps(rate)) - 1) // 2) // R0 + 1, NSAMP * (rate_mid // 12000))


def _reference(mod, xv, iq, rate, f_dial_hz, gain):
    """reference() of `mod` (this module or ddc_rat: its plan, frequency words, _mid and mid_count) on sample values"""
    rate_mid = mod.plan(rate)[0]
    if len(xv) > 15 * rate:
        raise _lib.Ft8rxError(f"x: {len(xv)} samples > {15 * rate} (15 s at {rate} Hz)")
    _, _, dial_mid, f_mixed = mod.frequency_words(rate, f_dial_hz)
    v = mod._mid(xv, iq, rate, f_dial_hz, 0, mod.mid_count(len(xv), rate), 0)
    y, _ = _ddc.reference(v, _ddc.IQ_F32, rate_mid, dial_mid, gain)
    return y, f_mixed


def reference(x, kind, rate, f_dial_hz, gain=1.0):
    """The float64 twin of the whole chain for one cycle and one channel -> (y float64 [180000], f_mixed_hz): the pre-stage, then
    ddc.reference on its output as an IQ stream at rate_mid with the dial f_dial - f0.  The frame is rint(y) saturated to int16."""
    return _reference(sys.modules[__name__], sample_values(x, kind), is_iq(kind), rate, f_dial_hz, gain)


def _reference_stream(mod, x, kind, rate, f_dial_hz, m_lo, m_hi, n_origin, k_origin, gain):
    """reference_stream() of `mod` behind its checks of the origin, whose intermediate sample is k_origin"""
    rate_mid = mod.plan(rate)[0]
    D = rate_mid // 12000
    dial_mid = mod.frequency_words(rate, f_dial_hz)[2]
    h1, h2 = _ddc.taps(rate_mid, 1), _ddc.taps(rate_mid, 2)
    reach = (len(h2) - 1) // 2 * (D // 2) + (len(h1) - 1) // 2             # intermediate samples an output reaches each way
    k_lo, k_hi = max(m_lo * D - reach, k_origin), (m_hi - 1) * D + reach + 1
    if k_hi <= k_lo:
        return np.zeros(m_hi - m_lo)
    v = mod._mid(mod.sample_values(x, kind), mod.is_iq(kind), rate, f_dial_hz, k_lo, k_hi, n_origin)
    # the intermediate stream is zero before k_origin and the outputs asked for reach nothing before k_lo: it may begin at k_lo
    return _ddc.reference_stream(v, _ddc.IQ_F32, rate_mid, dial_mid, m_lo, m_hi, n_origin=k_lo, gain=gain)


def reference_stream(x, kind, rate, f_dial_hz, m_lo, m_hi, n_origin=0, gain=1.0):
    """The float64 twin of the continuous definition: x[0] has the absolute index n_origin (a multiple of 1008 rate / 12000; zero before
    it and after the end of x) -> y float64 for the absolute 12 kHz outputs m_lo <= m < m_hi.  Only the intermediate samples those
    outputs reach are made; the second half is ddc.reference_stream, which begins at k_origin = n_origin / R0."""
    rate_mid, R0 = plan(rate)
    D = rate_mid // 12000
    m_lo, m_hi, n_origin = int(m_lo), int(m_hi), int(n_origin)
    if m_hi <= m_lo or n_origin < 0:
        raise _lib.Ft8rxError(f"outputs [{m_lo}, {m_hi}) / n_origin {n_origin}: need m_lo < m_hi and n_origin >= 0")
    if n_origin % (TILE * D * R0):
        raise _lib.Ft8rxError(f"n_origin {n_origin} is not a multiple of {TILE * D * R0} (1008 rate / 12000)")
    return _reference_stream(sys.modules[__name__], x, kind, rate, f_dial_hz, m_lo, m_hi, n_origin, n_origin // R0, gain)
