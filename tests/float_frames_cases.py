"""Shared inputs of tests/test_float_frames.py, tests/test_gpu_float_frames.py and tests/test_gpu_float_levels.py (float32 frames,
DESIGN.md section 18): the four integer-valued frames, the level and edge frames with full 24-bit mantissas, and the two-channel IQ
streams built from golden frames -- at full level and so quiet that every int16 frame the down-converter makes of them is zero.
Everything is built once and handed out unchanged."""
import numpy as np

import ddc_cases as cases
from conftest import load_golden

NSAMP = 180000
RATE = 48000
QUIET = 2.0 ** -20
CHANNELS = ("synth_000000", "test_08")        # the golden frame on channel a, on channel b
WIDE_RATE = 240000
WIDE_UP = 64                                  # the quiet wide stream times this is its full-level form, exactly, in int16
_cache = {}


def _once(key, make):
    if key not in _cache:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def runs_frame():
    """Runs of +32767, -32768 and -32767 of lengths 1 .. 4000, the two corners alternating sample by sample in between"""
    def make():
        a = np.zeros(NSAMP, np.int16)
        at, i = 0, 0
        for n in (1, 2, 3, 7, 480, 481, 1919, 3840, 4000) * 12:
            a[at:at + n] = (32767, -32768, -32767)[i % 3]
            at, i = at + n + (i % 2), i + 1                      # (a zero between some of the runs)
        a[at:at + 2000:2], a[at + 1:at + 2000:2] = 32767, -32768
        return a
    return _once("runs", make)


def int_frames():
    """int16 [4, 180000]: synth_000000, test_08, an all-zero frame, the runs frame"""
    return _once("int", lambda: np.stack([load_golden("synth_000000")[0], load_golden("test_08")[0], np.zeros(NSAMP, np.int16), runs_frame()]))


# ---- level frames: float32(float64(a) * c) of a golden frame.  No c is a power of two, so the mantissas are full: 24 significant bits
LEVELS = {"NORM": 0.7071 / 32768,             # the [-1, 1] convention of float audio
          "QUIET": 8.3e-10,                   # normalised audio 90 dB down
          "LOUD": 51234.5}                    # int32-scaled floats, peak about 1.7e9
EDGE = 30000.0                                # the edge samples, in int16 counts before the scaling
EDGE_BASE = {"QUIET": "synth_000000", "LOUD": "test_08", "NORM": "synth_000000"}
STAGE_ORDER = ("QUIET", "LOUD", "NORM")       # the stage batch: these edge frames, then the integer-valued test_08


def scaled(a, c):
    """float32(float64(a) * c): one rounding"""
    return (np.asarray(a, np.float64) * float(c)).astype(np.float32)


def level_frame(name, level):
    """float32 [180000]: the golden frame `name` at LEVELS[level]"""
    return _once(("level", name, level), lambda: scaled(load_golden(name)[0], LEVELS[level]))


def level_frames():
    """[(name, level, float32 [180000])]: the six level frames, CHANNELS x LEVELS"""
    return [(n, lv, level_frame(n, lv)) for lv in LEVELS for n in CHANNELS]


def edge_frame(level):
    """The level frame of EDGE_BASE[level] with its first two samples at +30000 c and its last two at -30000 c: what a zero mask
    that leaked would read, before the frame's start (its own head) or beyond sample 180 000 (the next frame's head)"""
    def make():
        a = load_golden(EDGE_BASE[level])[0].astype(np.float64)
        a[:2], a[-2:] = EDGE, -EDGE
        return scaled(a, LEVELS[level])
    return _once(("edge", level), make)


def stage_batch():
    """float32 [4, 180000]: QUIET edge, LOUD edge, NORM edge, integer-valued test_08.  A leak past sample 180 000 of the quiet frame
    reads the loud frame's start; a leak before a frame's start reads its own large first samples"""
    return _once("stage", lambda: np.stack([edge_frame(lv) for lv in STAGE_ORDER] + [load_golden("test_08")[0].astype(np.float32)]))


def offsets():
    return cases.offsets(RATE)


def full_stream():
    """complex64 [720000] at 48 kHz: CHANNELS[j] as a USB channel at offsets()[j], placed by its spectrum (ddc_cases._place), at the
    level of the golden frames; nothing is rounded to integers"""
    def make():
        n = NSAMP * RATE // 12000
        spec = np.zeros(n, np.complex128)
        for name, f_off in zip(CHANNELS, offsets()):
            cases._place(spec, load_golden(name)[0], f_off)
        return (np.fft.ifft(spec) * n / NSAMP).astype(np.complex64)
    return _once("full", make)


def quiet_stream():
    """full_stream() times 2^-20, exact in float32: every |y| of the down-converter stays under 0.04 counts"""
    return _once("quiet", lambda: full_stream() * np.float32(QUIET))


def wide_offsets():
    return -0.31 * WIDE_RATE, 0.22 * WIDE_RATE + 137.3


def wide_quiet_stream():
    """IQ int16 [3 600 000, 2] at 240 kHz whose 12 kHz channels sit below half a count: the clean signals of six known messages per
    channel (tests/ddc_stream_cases.py: frames 1 and 2, without their noise) at 0.02 counts each, placed by their spectra, plus a
    uniform dither of +-0.5 count on I and Q, rounded: a component is +-1 with the probability of its magnitude and 0 otherwise, so
    its mean is the signal and what the rounding adds is white.  A channel takes 6 kHz of the 240: the float64 twin finds max |y| =
    0.29 and an rms of 0.042 counts per channel (tests/test_float_frames.py asserts the bound), of which the six signals are 0.035."""
    def make():
        import ddc_stream_cases as live
        from pyft8_amd import synth
        n = NSAMP * WIDE_RATE // 12000
        spec = np.zeros(n, np.complex128)
        for i, f_off in zip((1, 2), wide_offsets()):
            clean = np.zeros(NSAMP)
            for k, w77 in enumerate(live.messages(i)[1]):
                w = synth.tones_to_wave(synth.tones79(int(w77)), 300.0 + 2400.0 * (k + 0.5) / 6)
                i0 = 6000 + 1200 * k                              # 0.5 .. 1.0 s into the cycle
                clean[i0:i0 + len(w)] += 0.02 * w / np.abs(w).max()
            a = np.fft.rfft(clean)[:NSAMP // 2].copy()
            a[1:] *= 2.0
            spec[(int(round(15.0 * f_off)) + np.arange(len(a))) % n] += a
        x = np.fft.ifft(spec) * n / NSAMP
        rng = np.random.Generator(np.random.Philox(key=0xF10A7))
        d = rng.random((n, 2)) - 0.5
        return np.rint(np.stack([x.real, x.imag], axis=1) + d).astype(np.int16)
    return _once("wide", make)
