"""Panorama (ft8rx_pan*, csrc/kernels/pan.hpp): the averaged power spectrum of ONE raw input stream at its own
rate and the count of samples at the converter's rails -- the float64 twin of the kernels, the index arithmetic of the stream
(csrc/pan_ring.hpp), the normalisation of the keyword panorama=, and the axes.  No GPU needed.

    v       the sample on the int16 scale (kinds.values); a real kind has zero imaginary part
    window  w covers the ABSOLUTE samples [w N, (w + 1) N); only complete windows count
    X_w[k]  = sum_i win[i] v[w N + i] e^(-2 pi i ik / N), win = the periodic Hann window rounded to float32 (window)
    p_w[k]  = Re^2 + Im^2
    row     r = the windows [r A, (r + 1) A): P_r[j] = sum_w p_w[k(j)], a SUM (db divides); only rows that lie in the stream exist
    bins    IQ kinds: N, ascending frequency, j = bin (j + N / 2) mod N; real kinds: N / 2, j = k (the Nyquist bin is dropped)
    stats   per row (samples with a component at the format's lowest or highest code, the largest |c| in kinds.components' units);
            None for the float kinds, which have no rails
"""
import numpy as np

from . import _lib
from . import kinds as _k

KINDS, KIND_NAMES, _DTYPE = _k.view((_k.REAL_I16, _k.REAL_F32, _k.IQ_I16, _k.IQ_F32, _k.WIDE_REAL_I16, _k.WIDE_IQ_I16, _k.WIDE_IQ_U8, _k.WIDE_IQ_I8))
FFT_DEFAULT, MIN_FFT, MAX_FFT, MAX_AVG = 2048, 256, 8192, 65536           # FT8RX_PAN_*
ROWS_DEFAULT, MAX_ROWS = 256, 65536
PERIOD_DEFAULT_S = 0.16                                                    # one FT8 symbol per row


def _kind(kind):
    if kind not in KINDS:
        raise _lib.Ft8rxError(f"panorama: kind={kind!r} is none of the sample kinds {sorted(KINDS)}")
    return kind


def _int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check(n_fft=FFT_DEFAULT, n_avg=1, rows=ROWS_DEFAULT):
    """-> (n_fft, n_avg, rows) as ft8rx_pan_stream_open takes them; anything outside the definition is refused, naming the argument"""
    if not _int(n_fft) or not MIN_FFT <= int(n_fft) <= MAX_FFT or int(n_fft) & (int(n_fft) - 1):
        raise _lib.Ft8rxError(f"panorama: n_fft={n_fft!r}: a power of two in [{MIN_FFT}, {MAX_FFT}]")
    if not _int(n_avg) or not 1 <= int(n_avg) <= MAX_AVG:
        raise _lib.Ft8rxError(f"panorama: n_avg={n_avg!r}: an integer in [1, {MAX_AVG}]")
    if not _int(rows) or not 1 <= int(rows) <= MAX_ROWS:
        raise _lib.Ft8rxError(f"panorama: rows={rows!r}: an integer in [1, {MAX_ROWS}]")
    return int(n_fft), int(n_avg), int(rows)


def n_avg_for(period_s, rate, n_fft):
    """the windows per row that come closest to period_s seconds: max(1, rint(period_s rate / n_fft))"""
    return max(1, int(np.rint(float(period_s) * float(rate) / int(n_fft))))


def params(panorama, rate):
    """The panorama= keyword -> None (off) or (n_fft, n_avg, rows): None / False = off; True = n_fft 2048, about 0.16 s per row, 256
    rows; a dict of n_fft, n_avg or period_s, rows."""
    if panorama is None or panorama is False:
        return None
    if panorama is True:
        panorama = {}
    if not isinstance(panorama, dict):
        raise _lib.Ft8rxError(f"panorama={panorama!r}: None, True or a dict of n_fft, n_avg or period_s, rows")
    bad = set(panorama) - {"n_fft", "n_avg", "period_s", "rows"}
    if bad:
        raise _lib.Ft8rxError(f"panorama: unknown key(s) {sorted(bad)}; known are n_fft, n_avg, period_s, rows")
    if "n_avg" in panorama and "period_s" in panorama:
        raise _lib.Ft8rxError("panorama: n_avg and period_s both given -- one of them says how long a row is")
    n_fft = check(panorama.get("n_fft", FFT_DEFAULT))[0]
    if "n_avg" in panorama:
        n_avg = panorama["n_avg"]
    else:
        period = panorama.get("period_s", PERIOD_DEFAULT_S)
        if isinstance(period, bool) or not isinstance(period, (int, float, np.integer, np.floating)) or not period > 0:
            raise _lib.Ft8rxError(f"panorama: period_s={period!r}: a positive number of seconds")
        n_avg = n_avg_for(period, rate, n_fft)
    return check(n_fft, n_avg, panorama.get("rows", ROWS_DEFAULT))


def one_stream(panorama, n_streams):
    """more than one stream is refused, naming the keyword and the count"""
    if panorama is not None and panorama is not False and n_streams != 1:
        raise _lib.Ft8rxError(f"panorama: {n_streams} streams -- the panorama takes one stream")


def window(n_fft):
    """the periodic Hann window, computed in double and rounded once to float32 (= ft8rx_pan_window)"""
    n_fft = check(n_fft)[0]
    return (0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft))).astype(np.float32)


def bins(kind, n_fft):
    return int(n_fft) if _k.is_iq(_kind(kind)) else int(n_fft) // 2


def freqs(kind, rate, n_fft):
    """the frequency of every output bin in Hz: IQ (j - N / 2) rate / N, real k rate / N"""
    n = check(n_fft)[0]
    j = np.arange(bins(kind, n), dtype=np.float64)
    return (j - n // 2) * (float(rate) / n) if _k.is_iq(kind) else j * (float(rate) / n)


def rows_done(n_origin, n_end, n_fft, n_avg):
    """-> (r_first, r_done): the first row of a stream that began at n_origin, and the first row that is not complete once the samples
    [n_origin, n_end) exist (csrc/pan_ring.hpp: r_first, rows_done; = ft8rx_pan_rows_done)"""
    n_origin, n_end, N, A = int(n_origin), int(n_end), int(n_fft), int(n_avg)
    r_first = -(-(-(-n_origin // N)) // A)
    return r_first, max(n_end // N, r_first * A) // A


def held(n_origin, n_end, n_fft, n_avg, n_rows):
    """the finished rows [r_lo, r_hi) a ring of n_rows holds (csrc/pan_ring.hpp: held)"""
    r_first, r_hi = rows_done(n_origin, n_end, n_fft, n_avg)
    return max(r_first, r_hi - int(n_rows)), r_hi


def pack(samples, kind):
    """One stream's samples as the C-contiguous array ft8rx_pan takes -> (array, n): a real kind [n], an IQ kind (I, Q) pairs [n, 2],
    IQ float32 also complex [n]."""
    return _k.pack_stream(samples, _kind(kind), "panorama: ONE stream of {name} samples, {form}, got shape {shape}",
                          "panorama: kind {kind} needs integers in the {dtype} range, got dtype {got}")


def _rows(a, kind, n_fft, n_avg):
    """packed samples of whole rows -> (rows float64 [R, bins], stats int64 [R, 2] or None)"""
    N, A = n_fft, n_avg
    R = len(a) // (N * A)
    iq = _k.is_iq(kind)
    if R == 0:
        return np.zeros((0, bins(kind, N))), (np.zeros((0, 2), np.int64) if _k.is_integer(kind) else None)
    a = a[:R * A * N]
    v = _k.values(a, kind).reshape(R * A, N)
    X = np.fft.fft(v * window(N).astype(np.float64)[None, :], axis=1)
    p = X.real ** 2 + X.imag ** 2
    p = np.fft.fftshift(p, axes=1) if iq else p[:, :N // 2]
    rows = np.stack([p[r * A:(r + 1) * A].sum(axis=0) for r in range(R)])
    if not _k.is_integer(kind):
        return rows, None
    info = np.iinfo(_DTYPE[kind])
    rail = ((a == info.min) | (a == info.max)).reshape(R, N * A, -1).any(axis=2).sum(axis=1)
    peak = np.abs(_k.components(a, kind)).reshape(R, -1).max(axis=1)
    return rows, np.stack([rail, peak], axis=1).astype(np.int64)


def reference(samples, kind, n_fft=FFT_DEFAULT, n_avg=1, n_origin=0):
    """The panorama of the whole stream at once (the definition) -> (rows float64 [R, bins], stats int64 [R, 2] or None for a float
    kind): the rows r_first .. r_done - 1 of rows_done(n_origin, n_origin + n, ...)."""
    N, A, _ = check(n_fft, n_avg)
    a, n = pack(samples, kind)
    r_first, r_done = rows_done(n_origin, int(n_origin) + n, N, A)
    at = r_first * A * N - int(n_origin)
    return _rows(a[at:at + (r_done - r_first) * A * N] if r_done > r_first else a[:0], kind, N, A)


def reference_stream(chunks, kind, n_fft=FFT_DEFAULT, n_avg=1, n_origin=0):
    """The stream pushed chunk by chunk -> one (r_first, rows, stats) per push: the rows that push completed, the first of them being
    row r_first.  Their concatenation equals reference() of the concatenation."""
    N, A, _ = check(n_fft, n_avg)
    n_origin = int(n_origin)
    have = None
    out, done = [], rows_done(n_origin, n_origin, N, A)[1]
    for ch in chunks:
        a = pack(ch, kind)[0]
        have = a if have is None else np.concatenate([have, a])
        new = rows_done(n_origin, n_origin + len(have), N, A)[1]
        out.append((done,) + _rows(have[done * A * N - n_origin:new * A * N - n_origin] if new > done else have[:0], kind, N, A))
        done = new
    return out


def full_scale(kind, n_fft):
    """|X| of a full-scale tone in one window: an IQ exponential of amplitude 32768 gives 32768 N / 2, a real sine half of that"""
    return 32768.0 * int(n_fft) / 2.0 * (1.0 if _k.is_iq(_kind(kind)) else 0.5)


def db(rows, kind, n_fft, n_avg):
    """rows (sums of n_avg powers) -> dB relative to a full-scale tone of the kind; an empty bin gives -inf"""
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(np.asarray(rows, np.float64) / (int(n_avg) * full_scale(kind, n_fft) ** 2))
