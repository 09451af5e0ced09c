"""Down-converter: real or IQ input at 12 D kHz (D = 1, 2, 4, 8, 16) -> 12 kHz USB audio frames.

The GPU stage is ft8rx_ddc (Handle.ddc, Receiver.decode_stream).  Here: the taps the kernels use (from the library, the single source
of the tables), the float64 twin of the definition, and a wav reader for real (mono) and IQ (stereo) recordings."""
import numpy as np

from . import _lib
from . import kinds as _k
from .kinds import REAL_I16, REAL_F32, IQ_I16, IQ_F32  # noqa: F401 -- this module's kinds: include/ft8rx.h FT8RX_DDC_*

KINDS, KIND_NAMES, _DTYPE = _k.view((REAL_I16, REAL_F32, IQ_I16, IQ_F32))
RATES = tuple(12000 * d for d in (1, 2, 4, 8, 16))
NSAMP = _lib.NSAMP


def is_iq(kind):
    return kind in KINDS and _k.is_iq(kind)


def kind_of(samples, iq):
    """The kind of an array by its dtype: with iq IQ float32 for complex or float samples and IQ int16 for the rest, without it real
    int16 for integers and real float32 for the rest.  Complex samples without iq are refused."""
    a = np.asarray(samples)
    cplx = np.iscomplexobj(a)
    if cplx and not iq:
        raise _lib.Ft8rxError("samples are complex: pass iq=True")
    if iq:
        return IQ_F32 if cplx or a.dtype.kind == "f" else IQ_I16
    return REAL_I16 if a.dtype.kind in "iu" else REAL_F32


def decimation(rate):
    """D of a supported rate; anything else is refused."""
    if rate not in RATES:
        raise _lib.Ft8rxError(f"rate {rate} is not one of {RATES}")
    return int(rate) // 12000


def taps(rate, stage):
    """float32 taps of stage 1 (rate -> 24 kHz; empty below 48 kHz) or 2 (-> 12 kHz) at `rate`, as the kernels use them (ft8rx_ddc_taps)."""
    buf = np.zeros(512, np.float32)
    n = _lib.lib().ft8rx_ddc_taps(int(rate), int(stage), buf.ctypes.data, len(buf))
    if n < 0:
        raise _lib.Ft8rxError(f"ddc.taps: no filter for rate {rate} / stage {stage} (rates {RATES}, stages 1 and 2)")
    return buf[:n].copy()


def frequency_word(rate, f_dial_hz):
    """(w, f_mixed_hz): the mixer's 32-bit frequency word for a dial `f_dial_hz` from the stream's centre, and the dial it really mixes."""
    w = int(np.rint((float(f_dial_hz) + 3000.0) / float(rate) * 4294967296.0)) % (1 << 32)
    f = w * float(rate) / 4294967296.0 - 3000.0
    return w, f - rate if f >= 0.5 * rate else f


def as_complex(x, kind):
    """One stream's samples as complex128: real kinds [n]; IQ kinds complex [n] or (I, Q) pairs [n, 2]."""
    x = np.asarray(x)
    if is_iq(kind) and not np.iscomplexobj(x):
        if x.ndim != 2 or x.shape[1] != 2:
            raise _lib.Ft8rxError(f"x: {KIND_NAMES[kind]} samples are complex [n] or (I, Q) pairs [n, 2], got shape {x.shape}")
        x = x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)
    if x.ndim != 1 or (not is_iq(kind) and np.iscomplexobj(x)):
        raise _lib.Ft8rxError(f"x: {KIND_NAMES[kind]} samples of one stream, got shape {x.shape} {x.dtype}")
    return x.astype(np.complex128)


def _centred(x, h, step, k_lo, k_hi):
    """sum_j h[j] x[k step + j - c], c = (len(h) - 1) / 2, for k = k_lo .. k_hi - 1; x is zero outside its array (h is symmetric)."""
    h = h.astype(np.float64)
    if len(h) <= 64:
        full = np.convolve(x, h)
    else:                                              # a long filter: the same sums by FFT (error ~1e-16 of the largest term)
        n = len(x) + len(h) - 1
        nfft = 1 << (n - 1).bit_length()
        full = np.fft.ifft(np.fft.fft(x, nfft) * np.fft.fft(h, nfft))[:n]
    idx = np.arange(k_lo, k_hi) * step + (len(h) - 1) // 2
    ok = (idx >= 0) & (idx < len(full))
    out = np.zeros(len(idx), np.complex128)
    out[ok] = full[idx[ok]]
    return out


def reference(x, kind, rate, f_dial_hz, gain=1.0):
    """The float64 twin of the definition for one stream and one output, with the library's float32 taps and the same frequency word
    -> (y float64 [180000], f_mixed_hz).  The frame is rint(y) saturated to int16."""
    if kind not in (REAL_I16, REAL_F32, IQ_I16, IQ_F32):
        raise _lib.Ft8rxError(f"kind {kind} is not one of REAL_I16, REAL_F32, IQ_I16, IQ_F32")
    D = decimation(rate)
    if kind == REAL_I16 and D == 1:
        raise _lib.Ft8rxError("kind real int16 at rate 12000 is a frame already")
    if not -0.5 * rate <= f_dial_hz < 0.5 * rate:
        raise _lib.Ft8rxError(f"f_dial_hz {f_dial_hz} outside [-rate / 2, rate / 2)")
    x = as_complex(x, kind)
    if len(x) > NSAMP * D:
        raise _lib.Ft8rxError(f"x: {len(x)} samples > {NSAMP * D} (15 s at {rate} Hz)")
    w, f_mixed = frequency_word(rate, f_dial_hz)
    phase = (np.arange(len(x), dtype=np.uint64) * np.uint64(w)) & np.uint64(0xFFFFFFFF)          # exact: n < 2^22, w < 2^32
    v = x * np.exp(-2j * np.pi * (phase.astype(np.float64) / 4294967296.0))
    h1, h2 = taps(rate, 1), taps(rate, 2)
    r2 = 1 if D == 1 else 2
    pad = len(h2) + 1                                  # even; the array of v starts at index -pad (stage 2 reaches back (len(h2) - 1) / 2)
    if len(h1):
        v = _centred(v, h1, D // 2, -pad, NSAMP * r2 + pad)
    else:
        v = np.concatenate([np.zeros(pad, np.complex128), v, np.zeros(NSAMP * r2 + pad - len(v), np.complex128)])
    z = _centred(v, h2, r2, pad // r2, pad // r2 + NSAMP)
    m = np.arange(NSAMP)
    g = 1.0 if is_iq(kind) else 2.0
    y = float(gain) * g * np.real(z * (1j ** (m % 4)))
    return y, f_mixed


def _stream_z(x, kind, rate, f_dial_hz, m_lo, m_hi, n_origin):
    """z[m] (complex128) of the continuous definition for the absolute outputs m_lo <= m < m_hi; x[0] is absolute input n_origin."""
    if kind not in (REAL_I16, REAL_F32, IQ_I16, IQ_F32):
        raise _lib.Ft8rxError(f"kind {kind} is not one of REAL_I16, REAL_F32, IQ_I16, IQ_F32")
    D = decimation(rate)
    if kind == REAL_I16 and D == 1:
        raise _lib.Ft8rxError("kind real int16 at rate 12000 is a frame already")
    if not -0.5 * rate <= f_dial_hz < 0.5 * rate:
        raise _lib.Ft8rxError(f"f_dial_hz {f_dial_hz} outside [-rate / 2, rate / 2)")
    m_lo, m_hi, n_origin = int(m_lo), int(m_hi), int(n_origin)
    if m_hi <= m_lo or n_origin < 0:
        raise _lib.Ft8rxError(f"outputs [{m_lo}, {m_hi}) / n_origin {n_origin}: need m_lo < m_hi and n_origin >= 0")
    x = as_complex(x, kind)
    w, _ = frequency_word(rate, f_dial_hz)
    h1, h2 = taps(rate, 1), taps(rate, 2)
    r2 = 1 if D == 1 else 2
    r1 = D // r2
    c1, c2 = (len(h1) - 1) // 2 if len(h1) else 0, (len(h2) - 1) // 2
    pad2 = c2 // r2 + 2                                 # v is taken for k_a <= k < k_b, k_a = (m_lo - pad2) r2: stage 2 reaches c2 each way
    k_a, k_b = (m_lo - pad2) * r2, (m_hi + pad2) * r2
    pad1 = c1 // r1 + 2                                 # u for n_a <= n < n_b, n_a = (k_a - pad1) r1
    n_a, n_b = (k_a - pad1) * r1, (k_b + pad1) * r1
    u = np.zeros(n_b - n_a, np.complex128)              # the input is zero before the origin and after the last sample
    lo, hi = max(n_a, n_origin), min(n_b, n_origin + len(x))
    if hi > lo:
        n = np.arange(lo, hi, dtype=np.uint64)
        phase = ((n & np.uint64(0xFFFFFFFF)) * np.uint64(w)) & np.uint64(0xFFFFFFFF)          # exact: both factors below 2^32
        u[lo - n_a:hi - n_a] = x[lo - n_origin:hi - n_origin] * np.exp(-2j * np.pi * (phase.astype(np.float64) / 4294967296.0))
    v = _centred(u, h1, r1, pad1, pad1 + k_b - k_a) if len(h1) else u[pad1 * r1:pad1 * r1 + k_b - k_a]
    return _centred(v, h2, r2, pad2, pad2 + m_hi - m_lo)


def reference_stream(x, kind, rate, f_dial_hz, m_lo, m_hi, n_origin=0, gain=1.0):
    """The float64 twin of the continuous definition: input of any length whose first sample x[0] has the
    absolute index n_origin (zero before it and after its end) -> y float64 for the absolute outputs m_lo <= m < m_hi.  n_origin sets
    the mixer phase (w n mod 2^32, exact at any n) and, through m, i^m.  Taps, frequency word and gain are reference's."""
    z = _stream_z(x, kind, rate, f_dial_hz, m_lo, m_hi, n_origin)
    m = np.arange(int(m_lo), int(m_hi))
    g = 1.0 if is_iq(kind) else 2.0
    return float(gain) * g * np.real(z * (1j ** (m % 4)))


def iq_from_wav(path):
    """A 16-bit .wav at a supported rate -> (samples, kind, rate): mono = real int16 [n] (REAL_I16), stereo = IQ with I left and Q
    right, int16 [n, 2] (IQ_I16).  (receiver.frames_from_wav reads finished 12 kHz frames.)"""
    import wave
    with wave.open(path, "rb") as w:
        channels, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        if width != 2:
            raise _lib.Ft8rxError(f"{path}: sample width {8 * width} bit, need 16")
        if channels not in (1, 2):
            raise _lib.Ft8rxError(f"{path}: channels {channels}, need 1 (real) or 2 (I, Q)")
        if rate not in RATES or (channels == 1 and rate == 12000):
            raise _lib.Ft8rxError(f"{path}: rate {rate} Hz with {channels} channel(s), need one of {RATES}"
                                  " (mono 12 kHz is a frame already: receiver.frames_from_wav)")
        x = np.frombuffer(w.readframes(n), dtype="<i2")
    if channels == 2:
        return x.reshape(-1, 2).copy(), IQ_I16, rate
    return x.copy(), REAL_I16, rate


def pack(samples, kind):
    """[n_streams][n] samples (one stream may come without the first axis) as the C-contiguous array ft8rx_ddc takes for `kind`
    -> (array, n_streams, n).  IQ: complex [n_streams, n] or pairs [n_streams, n, 2]."""
    if kind not in (REAL_I16, REAL_F32, IQ_I16, IQ_F32):
        raise _lib.Ft8rxError(f"kind {kind} is not one of REAL_I16, REAL_F32, IQ_I16, IQ_F32")
    a = np.asarray(samples)
    if is_iq(kind):
        if np.iscomplexobj(a):
            if kind == IQ_I16:
                raise _lib.Ft8rxError("samples: IQ int16 comes as (I, Q) pairs [n_streams, n, 2] of int16")
            a = np.ascontiguousarray(a[None] if a.ndim == 1 else a, np.complex64)
            a = a.view(np.float32).reshape(a.shape + (2,))
        elif a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[2] != 2:
            raise _lib.Ft8rxError(f"samples: {KIND_NAMES[kind]} needs complex [n_streams, n] or pairs [n_streams, n, 2], got shape {a.shape}")
    else:
        if np.iscomplexobj(a):
            raise _lib.Ft8rxError(f"samples: {KIND_NAMES[kind]} samples are real")
        if a.ndim == 1:
            a = a[None]
        if a.ndim != 2:
            raise _lib.Ft8rxError(f"samples: {KIND_NAMES[kind]} needs [n_streams, n], got shape {a.shape}")
    a = _k.as_dtype(a, kind, "samples: {name} needs integers in the {dtype} range")
    return a, a.shape[0], a.shape[1]
