"""Shared inputs of tests/test_report_cases.py and tests/test_gpu_report_edges.py: crafted calls of the report measurement (DESIGN.md
section 14) at the edges of its domain -- the borders of the 41 x 15 scan, the first and the last valid slice of the spectrum, the two
ends of the 3200-sample series, both sides of SWITCH, INVALID positions, an all-zero spectrum.  Nothing here touches a GPU; everything
is built once and handed out read-only.

A case is (name, spectrum index, f0_idx, h0_idx, ttweak, ftweak, word, expected flags); the part of the name before the first "/" is
its family.  The expected flags are the designed ones: tests/test_report_cases.py holds the float64 twin (pyft8_amd/report.py) to them,
and shows that no case is a near tie or moves under a dither of float32 size, so that the GPU test can leave out nothing.

Spectra of the default layout (49152 bins), all from synth.frame_with_signals through oracle.cycle_spectrum:
  0, 1    one signal at 1000 Hz, t0 = 0.5 s, at -10 dB and at +20 dB (on / off = 35 and 47 000: either side of SWITCH = 300); found at
          (f0_idx 320, h0_idx 12, ttweak 4, ftweak 0).  Spectrum 0 also carries a signal at 4500 Hz, which only the wide layout sees
  2, 3    zero but for the 1000 bins spec[fb - 150 : fb + 850] of spectrum 0 resp. 1, copied to the first and to the last 1000 bins
  4 .. 9  one signal at 1500 Hz at 0 dB starting at -5.6, -5.55, -2.0, 4.0, 7.0 and 8.8 s: 35 symbols before sample 0 of the series
          (h0_idx -140 is FT8RX_MIN_H0_FD) -- exact zeros of the zero fill among the noise cells, off > 0 -- then ten symbols past the end
          of the audio, and so late (h0_idx 220 = FT8RX_MAX_H0_FD) that more than half of the noise cells taken are zeros: off = 0 and
          the SNR sits on its floor.  Which cells are taken depends on the tones: SERIES_WORD picks a word for each
  10      all zero
The wide layout (96000 bins) has its own four: the audio of 0 and 1 through the wide transform, and their slices at its two ends."""
import numpy as np

import oracle as O
from pyft8_amd import _lib, synth
from pyft8_amd import report as R

M, INV, ET, EF = R.MEASURED, R.INVALID, R.EDGE_T, R.EDGE_F
WORDS = [synth.pack77("K1ABC", "W9XYZ", "-05"),          # bits above bit 63 set (the first call sits in bits 49 .. 76)
         synth.pack77("CQ", "G4XYZ", "IO91"),
         synth.pack77_ext("TNX BOB 73 GL"),              # free text: not a standard type
         synth.pack77("JA1XYZ", "VE3ABC", "RR73"),
         synth.pack77("EA5XYZ", "OH2ABC", "R-12")]
F0_1000, H0, TT = 320, 12, 4                             # where the 1000-Hz signals of spectra 0 and 1 are found (tb = 100, fb = 16000)
F0_1500, F0_4500 = 480, 1440
SERIES_T0 = [-5.6, -5.55, -2.0, 4.0, 7.0, 8.8]
SERIES_AT = [(-140, 0), (-139, 1), (-50, -1), (100, 0), (175, 0), (220, 0)]      # (h0_idx, ttweak): tb = 200 t0 for each (one more for the first)
SERIES_WORD = [0, 4, 3, 2, 0, 0]                         # chosen so that the first four keep off > 0 and the last two do not
N_AUDIO = 2 + len(SERIES_T0)

_cache = {}


def _ro(a):
    a.setflags(write=False)
    return a


def family(name):
    return name.split("/")[0]


def audio():
    """int16 [8, 180000]: the frames behind spectra 0, 1 and 4 .. 9."""
    if "audio" not in _cache:
        fr = [synth.frame_with_signals(31000, [(WORDS[0], 1000.0, 0.5, -10.0), (WORDS[3], 4500.0, 0.7, 3.0)]),
              synth.frame_with_signals(31001, [(WORDS[1], 1000.0, 0.5, 20.0)])]
        fr += [synth.frame_with_signals(31010 + k, [(WORDS[SERIES_WORD[k]], 1500.0, t0, 0.0)]) for k, t0 in enumerate(SERIES_T0)]
        _cache["audio"] = _ro(np.stack(fr))
    return _cache["audio"]


def _ends(src, bins):
    e = np.zeros(bins, np.complex64)
    sl = src[50 * F0_1000 - 150:50 * F0_1000 + 850]
    e[:1000] = sl
    e[bins - 1000:] = sl
    return e


def spectra(wide=False):
    """complex64 [11, 49152], or [4, 96000] for the wide layout."""
    key = ("spectra", bool(wide))
    if key not in _cache:
        a = audio()
        if wide:
            cfg = O.default_config(f0_hi=_lib.MAX_F0_WIDE)
            s = [O.cycle_spectrum(a[k], cfg) for k in range(2)]
            s += [_ends(s[0], _lib.SPEC_BINS_WIDE), _ends(s[1], _lib.SPEC_BINS_WIDE)]
        else:
            s = [O.cycle_spectrum(a[k]) for k in range(N_AUDIO)]
            s = s[:2] + [_ends(s[0], _lib.SPEC_BINS), _ends(s[1], _lib.SPEC_BINS)] + s[2:] + [np.zeros(_lib.SPEC_BINS, np.complex64)]
        _cache[key] = _ro(np.stack(s))
        assert _cache[key].shape == ((4, _lib.SPEC_BINS_WIDE) if wide else (11, _lib.SPEC_BINS))
    return _cache[key]


def _common(bins):
    """The families that both layouts run: interior, the borders of the scan, the ends of the spectrum."""
    last = bins - 850                                      # the last valid fb: 49152 - 850 = 50 * 966 + 2, 96000 - 850 = 50 * 1903
    f_hi, t_hi = last // 50, last % 50
    c = []
    for s, lvl in ((0, "lo"), (1, "hi")):
        w = WORDS[s]
        c.append((f"interior/{lvl}", s, F0_1000, H0, TT, 0, w, M))
        # the true start outside tau = tb - 28 .. tb + 12: the peak stays on the border; +28 / -12 put it exactly on the border
        c.append((f"tborder/{lvl}+40", s, F0_1000, H0, TT + 40, 0, w, M | ET))
        c.append((f"tborder/{lvl}-24", s, F0_1000, H0, TT - 24, 0, w, M | ET))
        # (the +20 dB signal peaks half a sample later, at tau = 101: with +28 that is cell 1, the first interior one)
        c.append((f"tborder/{lvl}+28", s, F0_1000, H0, TT + 28, 0, w, M | ET if s == 0 else M))
        c.append((f"tborder/{lvl}-12", s, F0_1000, H0, TT - 12, 0, w, M | ET))
        # 90 bins = 0.9 tone spacings: delta beyond +-0.7; 70 bins: exactly on the border
        c.append((f"fborder/{lvl}+90", s, F0_1000, H0, TT, 90, w, M | EF))
        c.append((f"fborder/{lvl}-90", s, F0_1000, H0, TT, -90, w, M | EF))
        c.append((f"fborder/{lvl}-70", s, F0_1000, H0, TT, -70, w, M | EF))
        c.append((f"bothborders/{lvl}", s, F0_1000, H0, TT + 40, 90, w, M | ET | EF))
        # the first and the last valid slice, and one bin further out on each side between them
        c.append((f"specend/{lvl}-first", 2 + s, 3, H0, TT, 0, w, M))
        c.append((f"invalid/{lvl}-below", 2 + s, 3, H0, TT, -1, w, M | INV))
        c.append((f"invalid/{lvl}-above", 2 + s, f_hi, H0, TT, t_hi + 1, w, M | INV))
        c.append((f"specend/{lvl}-last", 2 + s, f_hi, H0, TT, t_hi, w, M))
    return c


def cases(wide=False):
    """The cases of one layout, in the order the GPU test submits them: the INVALID ones stand between valid ones of their spectrum."""
    key = ("cases", bool(wide))
    if key not in _cache:
        if wide:
            c = _common(_lib.SPEC_BINS_WIDE)
            c.append(("interior/above3k", 0, F0_4500, 17, 4, 0, WORDS[3], M))
        else:
            c = _common(_lib.SPEC_BINS)
            c.insert(1, ("invalid/h0-below", 0, F0_1000, _lib.MIN_H0_FD - 1, TT, 0, WORDS[0], M | INV))
            c.insert(4, ("invalid/h0-above", 0, F0_1000, _lib.MAX_H0_FD + 1, TT, 0, WORDS[0], M | INV))
            for k, (t0, (h0, tt)) in enumerate(zip(SERIES_T0, SERIES_AT)):
                c.append((f"series/{t0:+.2f}s", 4 + k, F0_1500, h0, tt, 0, WORDS[SERIES_WORD[k]], M))
            c.append(("zero/h0+200", 10, 400, 200, 3, 7, WORDS[4], M | ET | EF))
            c.append(("zero/h0-50", 10, 700, -50, -2, -9, WORDS[2], M | ET | EF))
        assert len({x[0] for x in c}) == len(c)
        _cache[key] = tuple(c)
    return _cache[key]


# a spectrum-end case and the interior case it must equal in everything but f_hz
SAME_AS = {"specend/lo-first": "interior/lo", "specend/lo-last": "interior/lo", "specend/hi-first": "interior/hi", "specend/hi-last": "interior/hi"}
FLOOR_DB = 10.0 * np.log10(R.SNR_FLOOR * 6.25 / 2500.0)             # -56.02 dB
ON_FLOOR = ("series/+7.00s", "series/+8.80s", "zero/h0+200", "zero/h0-50")


def twin(wide=False):
    """name -> the float64 twin's result (None for INVALID), computed once per layout."""
    key = ("twin", bool(wide))
    if key not in _cache:
        sp = spectra(wide)
        _cache[key] = {n: R.measure(sp[s], f0, h0, tt, ft, w) for n, s, f0, h0, tt, ft, w, _ in cases(wide)}
    return _cache[key]


def columns(cs, frame_of=None):
    """The argument columns of Handle.report_probe for the cases cs; frame_of maps a spectrum index to a row of the spec array handed in."""
    fr = [c[1] if frame_of is None else frame_of[c[1]] for c in cs]
    return (fr, [c[2] for c in cs], [c[3] for c in cs], [c[4] for c in cs], [c[5] for c in cs], [c[6] for c in cs])
