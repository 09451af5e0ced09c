"""Rational resampler: ONE stream at an integer rate in [16000, 129600000] that neither ddc.RATES nor
ddc_wide.plan takes -- 44.1 kHz sound cards, RTL-SDR at 2.048 MS/s, HackRF at 10 MS/s -- in front of the down-converter of ddc.py.

The GPU stage is ft8rx_ddc_rat* (Handle.ddc_rat, Handle.ddc_rat_stream_*, Receiver.decode_stream(..., resample=True)).  Here: the kinds,
the plan of a rate and the taps of the prototype (both from the library, the single source), the frequency words, and the float64 twins
of the definition.  The twins make only the intermediate samples that are asked for, by direct dot products over the taps of each
sample's phase."""
import sys

import numpy as np

from . import _lib
from . import ddc as _ddc
from . import ddc_wide as _dw
from . import kinds as _k
from .kinds import REAL_I16, REAL_F32, IQ_I16, IQ_F32  # noqa: F401 -- include/ft8rx.h FT8RX_DDC_*

IQ_U8, IQ_I8 = _k.WIDE_IQ_U8, _k.WIDE_IQ_I8            # include/ft8rx.h FT8RX_WIDE_IQ_U8, FT8RX_WIDE_IQ_I8
KINDS, KIND_NAMES, _DTYPE = _k.view((REAL_I16, REAL_F32, IQ_I16, IQ_F32, IQ_U8, IQ_I8))
NSAMP = _lib.NSAMP
TILE = 1008
N_MAX = 1 << 52
_REFUSED = "outside [16000, 129600000], a rate of ddc or ddc_wide, L > 320 or more than 8448 taps"


def _kind(kind):
    if kind not in KINDS:
        raise _lib.Ft8rxError(f"kind {kind} is not one of REAL_I16, REAL_F32, IQ_I16, IQ_F32, IQ_U8, IQ_I8 (ddc_rat)")
    return kind


def is_iq(kind):
    return _k.is_iq(_kind(kind))


def kind_of(samples, iq):
    """The kind of an array by its dtype: complex64 / complex128 [n] is IQ float32; with iq, (I, Q) pairs [n, 2] of int16, float32,
    uint8 or int8; without, int16 or float32 / float64 [n].  Anything else is refused, naming the dtype."""
    a = np.asarray(samples)
    if a.dtype.kind == "c":
        return IQ_F32
    if a.dtype == np.int16:
        return IQ_I16 if iq else REAL_I16
    if a.dtype.kind == "f":
        return IQ_F32 if iq else REAL_F32
    if iq and a.dtype == np.uint8:
        return IQ_U8
    if iq and a.dtype == np.int8:
        return IQ_I8
    raise _lib.Ft8rxError(f"samples: dtype {a.dtype} is not taken (iq: complex, or int16 / float32 / uint8 / int8 pairs; real: int16 or float32)")


def accepts(rate):
    """True for a rate the resampler takes (ft8rx_ddc_rat_plan)."""
    try:
        return _lib.lib().ft8rx_ddc_rat_plan(int(rate), None, None, None, None) == 0
    except (TypeError, ValueError, OverflowError):
        return False


def plan(rate):
    """(rate_mid, L, M, N) of a rate: rate_mid = rate L / M is the one of 192000, 96000, 48000 with the smallest L (ties: the largest),
    N the length of the prototype; anything else is refused (ft8rx_ddc_rat_plan)."""
    v = np.zeros(4, np.int32)
    if not isinstance(rate, (int, np.integer)) or not -2 ** 31 <= rate < 2 ** 31 or \
            _lib.lib().ft8rx_ddc_rat_plan(int(rate), v[0:].ctypes.data, v[1:].ctypes.data, v[2:].ctypes.data, v[3:].ctypes.data) != 0:
        raise _lib.Ft8rxError(f"rate {rate} is not taken: {_REFUSED}")
    return int(v[0]), int(v[1]), int(v[2]), int(v[3])


def taps(rate):
    """float32 taps of the prototype h at `rate`, as the kernel uses them (ft8rx_ddc_rat_taps); sum h = L."""
    n = plan(rate)[3]
    buf = np.zeros(n, np.float32)
    if _lib.lib().ft8rx_ddc_rat_taps(int(rate), buf.ctypes.data, len(buf)) != n:
        raise _lib.Ft8rxError(f"ddc_rat.taps: no filter for rate {rate}")
    return buf


def frequency_words(rate, f_dial_hz):
    """(w0, f0, dial_mid, f_mixed_hz) of a dial `f_dial_hz` from the stream's centre: the resampler's 32-bit frequency word, the
    frequency it really mixes (in [-rate/2, rate/2)), the dial left for the down-converter behind it (f_dial - f0, about -3000 Hz) and
    the dial the whole chain really mixes."""
    return _dw._words(rate, plan(rate)[0], f_dial_hz)


def pack(samples, kind):
    """One stream's samples as the C-contiguous array ft8rx_ddc_rat takes for `kind` -> (array, n): real kinds [n]; IQ kinds (I, Q)
    pairs [n, 2] (IQ float32 also as complex [n])."""
    return _k.pack_stream(samples, _kind(kind), "samples: {name} is ONE stream, {form}, got shape {shape} {got}",
                          "samples: {name} needs integers in the {dtype} range, got dtype {got}")


def sample_values(x, kind):
    """One stream's samples as float64 [n] (real) or complex128 [n] (IQ): the 16-bit and float kinds as they are, uint8 u ->
    256 (u - 127.5), int8 s -> 256 s.  (The twins also take values that are on that scale already: float64 [n] for a real kind,
    complex [n] for an IQ kind.)"""
    a = np.asarray(x)
    if a.ndim == 1 and (a.dtype.kind == "c" if is_iq(kind) else a.dtype == np.float64):
        return a.astype(np.complex128 if is_iq(kind) else np.float64)
    return _k.values(pack(x, kind)[0], kind)


def phase_table(rate, w0=0):
    """T[phi][i] = h[phi + i L] e^{+2 pi i (w0 i mod 2^32) / 2^32}, i < P = ceil(N / L), zero from N on -> complex128 [L, P]"""
    _, L, _, N = plan(rate)
    P = -(-N // L)
    h = np.zeros(L * P)
    h[:N] = taps(rate).astype(np.float64)
    rot = np.conj(_dw._phasor((np.arange(P, dtype=np.uint64) * np.uint64(w0)) & np.uint64(0xFFFFFFFF)))
    return h.reshape(P, L).T * rot[None, :]


def _mid(xv, iq, rate, f_dial_hz, k_lo, k_hi, n_origin):
    """reference_mid on sample values (float64 real or complex128)"""
    _, L, M, N = plan(rate)
    if not -0.5 * rate <= f_dial_hz < 0.5 * rate:
        raise _lib.Ft8rxError(f"f_dial_hz {f_dial_hz} outside [-rate / 2, rate / 2)")
    k_lo, k_hi, n_origin = int(k_lo), int(k_hi), int(n_origin)
    if k_hi <= k_lo or k_lo < 0 or not 0 <= n_origin <= N_MAX:
        raise _lib.Ft8rxError(f"intermediate samples [{k_lo}, {k_hi}) / n_origin {n_origin}: need 0 <= k_lo < k_hi and 0 <= n_origin <= 2^52")
    C, P = (N - 1) // 2, -(-N // L)
    w0 = frequency_words(rate, f_dial_hz)[0]
    T = phase_table(rate, w0)
    t = np.arange(k_lo, k_hi, dtype=np.int64) * M + C                      # t_k = k M + C, below 2^62
    b, phi = t // L, t % L                                                 # the last input of k and its phase
    n_a, n_b = int(b[0]) - (P - 1), int(b[-1]) + 1                         # the inputs under the outputs asked for
    xs = np.zeros(n_b - n_a, xv.dtype)
    lo, hi = max(n_a, n_origin), min(n_b, n_origin + len(xv))
    if hi > lo:
        xs[lo - n_a:hi - n_a] = xv[lo - n_origin:hi - n_origin]
    v = np.empty(k_hi - k_lo, np.complex128)
    rows = max(1, (1 << 21) // P)
    back = np.arange(P, dtype=np.int64)
    for a in range(0, len(v), rows):
        idx = (b[a:a + rows] - n_a)[:, None] - back[None, :]               # x[b_k - i]
        v[a:a + rows] = np.einsum("ki,ki->k", T[phi[a:a + rows]], xs[idx])
    rot = _dw._phasor(((b % (1 << 32)).astype(np.uint64) * np.uint64(w0)) & np.uint64(0xFFFFFFFF))      # (w0 b_k) mod 2^32
    return (1.0 if iq else 2.0) * rot * v


def reference_mid(x, kind, rate, f_dial_hz, k_lo, k_hi, n_origin=0):
    """The float64 twin of the resampler alone: intermediate samples v[k], k_lo <= k < k_hi (absolute), of one channel -> complex128.
    x[0] has the absolute index n_origin; the stream is zero before it and after its end.  Library taps, exact integer phases."""
    return _mid(sample_values(x, kind), is_iq(kind), rate, f_dial_hz, k_lo, k_hi, n_origin)


def mid_count(n_samples, rate):
    """Intermediate samples of a one-shot call on n_samples inputs (csrc/ddc_rat_ring.hpp: mid_count)"""
    rate_mid, L, M, N = plan(rate)
    if n_samples < 1:
        return 1
    return min(((n_samples - 1) * L + (N - 1) // 2) // M + 1, NSAMP * (rate_mid // 12000))


def origin_ok(n_origin, rate):
    """True for a valid stream origin: k_origin = n_origin L / M is an integer multiple of 1008 rate_mid / 12000"""
    rate_mid, L, M, _ = plan(rate)
    n_origin = int(n_origin)
    return 0 <= n_origin <= N_MAX and (n_origin * L) % M == 0 and (n_origin * L // M) % (TILE * (rate_mid // 12000)) == 0


def reference(x, kind, rate, f_dial_hz, gain=1.0):
    """The float64 twin of the whole chain for one cycle and one channel -> (y float64 [180000], f_mixed_hz): the resampler, then
    ddc.reference on its output as an IQ stream at rate_mid with the dial f_dial - f0.  The frame is rint(y) saturated to int16."""
    return _dw._reference(sys.modules[__name__], sample_values(x, kind), is_iq(kind), rate, f_dial_hz, gain)


def reference_stream(x, kind, rate, f_dial_hz, m_lo, m_hi, n_origin=0, gain=1.0):
    """The float64 twin of the continuous definition: x[0] has the absolute index n_origin (a valid origin, origin_ok; zero before it
    and after the end of x) -> y float64 for the absolute 12 kHz outputs m_lo <= m < m_hi.  Only the intermediate samples those
    outputs reach are made; the second half is ddc.reference_stream, which begins at k_origin = n_origin L / M."""
    rate_mid, L, M, _ = plan(rate)
    D = rate_mid // 12000
    m_lo, m_hi, n_origin = int(m_lo), int(m_hi), int(n_origin)
    if m_hi <= m_lo:
        raise _lib.Ft8rxError(f"outputs [{m_lo}, {m_hi}): need m_lo < m_hi")
    if not origin_ok(n_origin, rate):
        raise _lib.Ft8rxError(f"n_origin {n_origin}: n_origin L / M must be an integer multiple of {TILE * D} (1008 rate_mid / 12000)")
    return _dw._reference_stream(sys.modules[__name__], x, kind, rate, f_dial_hz, m_lo, m_hi, n_origin, n_origin * L // M, gain)


def iq_from_wav(path):
    """A 16-bit .wav at a rate the resampler takes -> (samples, kind, rate): mono = real int16 [n] (REAL_I16), stereo = IQ with I left
    and Q right, int16 [n, 2] (IQ_I16).  (ddc.iq_from_wav reads the rates of ddc.RATES.)"""
    import wave
    with wave.open(path, "rb") as w:
        channels, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        if width != 2:
            raise _lib.Ft8rxError(f"{path}: sample width {8 * width} bit, need 16")
        if channels not in (1, 2):
            raise _lib.Ft8rxError(f"{path}: channels {channels}, need 1 (real) or 2 (I, Q)")
        if not accepts(rate):
            raise _lib.Ft8rxError(f"{path}: rate {rate} Hz is not taken: {_REFUSED}")
        x = np.frombuffer(w.readframes(n), dtype="<i2")
    if channels == 2:
        return x.reshape(-1, 2).copy(), IQ_I16, rate
    return x.copy(), REAL_I16, rate
