"""Measured signal reports (ft8rx_set_reports): the float64 numpy twin of kernels/report.hpp.

A message dict's "their_snr" / "fHz" / "tsec" are the reference's quantities: (pmax - pmin) - 58 clipped to +-24, and the position on
the search grid plus the tweaks.  Once a candidate has DECODED its 79 tones are known, so strength, frequency and start time can be
measured with a matched correlation over the whole signal instead.  measure() is the definition; the kernel k_report follows it
step by step in float32 and the tests compare the two on the same cycle spectrum."""
import numpy as np

from . import _lib, synth

NTAU, TAU_LO = 41, -28                     # tau = tb - 28 .. tb + 12 (5-ms samples of the 3200-sample series)
NDEL, DEL_STEP = 15, 0.1                   # delta = -0.7 .. +0.7 tone spacings (6.25 Hz)
HANN = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(32) + 0.5) / 32.0)
SNR_FLOOR = 1e-3                           # floor of on / off - 1
SWITCH, TOP_TONE = 300.0, 6                # on / off above which the noise cells of tones 6 and 7 are left out (see snr())
MEASURED, INVALID, EDGE_T, EDGE_F = 1, 2, 4, 8      # ft8rx_report.flags (include/ft8rx.h FT8RX_RP_*)


def series(spec, fb):
    """The 3200-sample series of the slice at bin fb (tests/test_fine_identity.py: _series): taper, 3200-point inverse FFT."""
    step = (0.0 - np.pi) / 99.0
    y = np.array([0.0 if i == 99 else i * step + np.pi for i in range(100)])
    taper = 0.5 * (1.0 + np.cos(y))
    X = np.zeros(3200, np.complex128)
    seg = spec[fb:fb + 850].astype(np.complex128); seg[750:] *= taper
    low = spec[fb - 150:fb].astype(np.complex128); low[:100] *= taper
    X[:850] = seg; X[3050:] = low
    return np.fft.ifft(X)


def _symbols(z, tau):
    """[79, 32]: the 32 samples of every symbol for a start at sample tau; samples outside the series are zero."""
    idx = tau + 32 * np.arange(79)[:, None] + np.arange(32)[None, :]
    ok = (idx >= 0) & (idx < 3200)
    return np.where(ok, z[np.clip(idx, 0, 3199)], 0.0)


def scan(z, tones, tb):
    """P[tau, delta] = sum_s |sum_n z[tau + 32 s + n] e^{-2 pi i n (tone_s + delta) / 32}|^2 -> [41, 15]"""
    n = np.arange(32)
    d = DEL_STEP * (np.arange(NDEL) - NDEL // 2)
    K = np.exp(-2j * np.pi * n[None, :, None] * (np.asarray(tones, float)[:, None, None] + d[None, None, :]) / 32.0)     # [79, 32, 15]
    X = np.stack([_symbols(z, tb + TAU_LO + i) for i in range(NTAU)], axis=1)                                         # [79, 41, 32]
    return (np.abs(X @ K) ** 2).sum(axis=0)


def _parabola(a, b, c):
    den = a - 2.0 * b + c
    return 0.5 * (a - c) / den if den != 0.0 else 0.0


def far_mask(tones):
    """[79, 8] bool: the cells of the 79 x 8 grid further than two tones from the tone of the symbol, of the one before and of the
    one after it -- where the Hann-weighted transform sees no signal."""
    t = np.asarray(tones, int)
    cell = np.arange(8)[None, :]
    keep = np.ones((79, 8), bool)
    for sh in (-1, 0, 1):
        s = np.arange(79) + sh
        ok = (s >= 0) & (s < 79)
        near = np.abs(cell - t[np.clip(s, 0, 78)][:, None]) <= 2
        keep &= ~(near & ok[:, None])
    return keep


def median(cells):
    """The middle of the sorted cells; the mean of the two middle ones for an even count (as the kernel selects them)."""
    c = np.sort(np.asarray(cells, float))
    m = len(c)
    return 0.5 * (c[(m - 1) // 2] + c[m // 2])


def snr(z, tones, tau, delta):
    """-> (snr_db, on, off) at the integer tau and the interpolated delta.  on = the mean rectangular |DFT|^2 at each symbol's own
    tone; off = the noise per rectangular cell, median / ln 2 * 32 / sum w^2 of the Hann-weighted cells away from the signal
    (far_mask).  A signal leaks into the two highest cells, next to the edge of the slice, 20 - 30 dB more than into the others (1e-4
    resp. 1e-5 of `on`): once on / off exceeds SWITCH that is no longer small against the noise, and off is taken again from the far
    cells of the tones 0 .. TOP_TONE - 1 alone."""
    n = np.arange(32)
    X = _symbols(z, tau)
    E = np.exp(-2j * np.pi * n[None, :] * (np.arange(8)[:, None] + delta) / 32.0)            # [8, 32]
    rect = np.abs(X @ E.T) ** 2                                                             # [79, 8]
    hann = np.abs((X * HANN[None, :]) @ E.T) ** 2
    on = float(rect[np.arange(79), np.asarray(tones, int)].mean())
    far = far_mask(tones)
    scale = 32.0 / float((HANN ** 2).sum()) / np.log(2.0)
    off = median(hann[far]) * scale if far.any() else 0.0
    if on > SWITCH * off and far[:, :TOP_TONE].any():
        off = median(hann[:, :TOP_TONE][far[:, :TOP_TONE]]) * scale
    ratio = on / off - 1.0 if off > 0.0 else SNR_FLOOR
    return 10.0 * np.log10(max(ratio, SNR_FLOOR) * 6.25 / 2500.0), on, off


def measure(spec, f0_idx, h0_idx, ttweak, ftweak, word):
    """The report of one DECODED record on its frame's cycle spectrum (complex [SPEC_BINS]) -> dict(snr_db, f_hz, t_sec, score,
    flags, P), or None for an invalid report (h0_idx outside the frequency-domain range, or a slice that leaves the spectrum)."""
    fb = 50 * int(f0_idx) + int(ftweak)
    if not _lib.MIN_H0_FD <= int(h0_idx) <= _lib.MAX_H0_FD or fb - 150 < 0 or fb + 850 > len(spec):
        return None
    tones = synth.tones79(int(word))
    z = series(np.asarray(spec), fb)
    tb = 8 * int(h0_idx) + (1 if h0_idx < 0 else 0) + int(ttweak)
    P = scan(z, tones, tb)
    it, idl = np.unravel_index(int(np.argmax(P)), P.shape)                  # the first maximum, tau-major
    flags = MEASURED
    dt = dd = 0.0
    if 0 < it < NTAU - 1:
        dt = _parabola(P[it - 1, idl], P[it, idl], P[it + 1, idl])
    else:
        flags |= EDGE_T
    if 0 < idl < NDEL - 1:
        dd = _parabola(P[it, idl - 1], P[it, idl], P[it, idl + 1])
    else:
        flags |= EDGE_F
    delta = DEL_STEP * (idl - NDEL // 2 + dd)
    tau = tb + TAU_LO + it
    snr_db, on, off = snr(z, tones, tau, delta)
    return dict(snr_db=snr_db, f_hz=0.0625 * fb + 6.25 * delta, t_sec=0.005 * (tau + dt), score=float(P[it, idl]), flags=flags,
                P=P, on=on, off=off)
