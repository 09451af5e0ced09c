"""Fixtures of the FT4 subtraction tests (tests/test_ft4_sub.py on the CPU, tests/test_gpu_ft4_sub.py on the GPU; DESIGN.md section
19.6): the crowded frames of the yield figures, noise-free cancellation cases, crafted probe signals and the batch of the residual
test.  Everything comes from pyft8_amd/ft4.py (the float64 twin) and seeds; nothing is read from disk, and what the twin computes is
computed once per process and shared."""
import functools

import numpy as np

from pyft8_amd import ft4, synth

# ---- the crowded frames: 16 signals in 900 Hz, -12 .. +10 dB; the figures of the float64 twin on them (tests/test_ft4_sub.py asserts
# them): pass 1 decodes 7 / 9 / 10 of the 16, a second pass after one subtraction sweep brings 10 / 15 / 14
CROWDED = (500, 501, 502)
CROWDED_KW = dict(n_signals=16, snr_range=(-12, 10), freq_range=(300, 1200), t0_range=(0.2, 1.2), min_sep_hz=25)
TWIN_PASS1, TWIN_TOTAL = 26, 39


@functools.lru_cache(maxsize=None)
def crowded(index):
    """-> (audio int16 [90000], truth)"""
    return ft4.make_frame(index, return_truth=True, **CROWDED_KW)


def words(n, seed=1):
    rng = np.random.Generator(np.random.Philox(key=ft4.SEED_BASE + 7700 + seed))
    return [synth.pack77(*ft4.random_message(rng)) for _ in range(n)]


def sig(word, f0_hz, start):
    """the signal record a decoder would hand over: fq on the 2.6-Hz grid (up to 1.3 Hz off), the given start"""
    return dict(start=int(start), fq=int(round(f0_hz / ft4.DF_HZ)), tones=ft4.tones105(word), word=int(word))


def subsig_array(sigs):
    from pyft8_amd import _lib
    a = np.zeros(len(sigs), _lib.FT4_SUBSIG_DTYPE)
    for i, s in enumerate(sigs):
        a[i]["start"], a[i]["fq"], a[i]["tones"] = s["start"], s["fq"], np.asarray(s["tones"], np.uint8)
    return a


# ---- cancellation: one noise-free signal, amplitude 1000
CANCEL = ((1000.3, 6000), (2503.9, -3600), (317.1, 29000), (5890.0, 24000))
CANCEL_OFFSETS = (-18, -7, 0, 5, 18)


@functools.lru_cache(maxsize=None)
def clean_frame(f0_hz, start, word=None):
    """-> (float64 [90000]: the part of the signal inside the frame, its word)"""
    word = words(1)[0] if word is None else word
    w = 1000.0 * ft4.tones_to_wave(ft4.tones105(word), f0_hz)
    x = np.zeros(ft4.NFRAME)
    a, b = max(0, start), min(ft4.NFRAME, start + len(w))
    x[a:b] = w[a - start:b - start]
    return x, word


# ---- the probe: crafted signals on three frames.  (frame, f0 Hz, true start, snr dB or None = nothing planted, offset of the given start)
# The offsets put the true start on a refine trial (a multiple of 4 within +-24) or one sample off it.
#   frame 0: noise and five signals -- the lowest and the highest tone-0 frequency of the search range, -14 dB, +10 dB, a winner at the
#            first trial; and a place where nothing was planted
#   frame 1: no noise -- a start at -0.3 s, a signal that runs past sample 89 999, one in the middle; two models wholly outside the frame
#   frame 2: all zero
PROBE = ((0, 21.7, 6000, 0.0, 4), (0, 5900.0, 9000, 0.0, -24), (0, 1500.3, 3000, -14.0, 12), (0, 2503.9, 12345, 10.0, -17),
         (0, 800.0, 1200, -5.0, 24), (0, 3600.0, 5000, None, 0),
         (1, 1000.3, -3600, 3.0, 5), (1, 317.1, 40000, 3.0, -20), (1, 3333.3, 24000, 3.0, 0), (1, 2000.0, -70000, None, 0), (1, 2000.0, 95000, None, 0),
         (2, 1302.1, 1000, None, 0))


@functools.lru_cache(maxsize=None)
def probe_cases():
    """-> (audio int16 [3][90000], frame [n], the signals as given to the decoder [n], the true starts [n] (None where nothing is planted))"""
    ws = words(len(PROBE), seed=2)
    planted = [[], [], []]
    for w, (f, f0, start, snr, _) in zip(ws, PROBE):
        if snr is not None:
            planted[f].append((w, f0, start / ft4.FS, snr))
    audio = np.stack([ft4.frame_with_signals(1, planted[0]), ft4.frame_with_signals(2, planted[1], noise=False), np.zeros(ft4.NFRAME, np.int16)])
    sigs = [sig(w, f0, start + off) for w, (_, f0, start, _, off) in zip(ws, PROBE)]
    truth = [start if snr is not None else None for _, _, start, snr, _ in PROBE]
    return audio, np.array([p[0] for p in PROBE], np.int32), sigs, truth


@functools.lru_cache(maxsize=None)
def probe_twin():
    """the twin on the probe cases -> (models complex [n][60480], bins [n][41], energies [n][13], refined starts [n])"""
    audio, frame, sigs, _ = probe_cases()
    models = [ft4.sub_model(s["tones"], s["fq"]) for s in sigs]
    x = audio.astype(np.float64)
    bins = np.array([ft4.sub_bins(x[f], s["start"], m) for f, s, m in zip(frame, sigs, models)])
    en = np.array([ft4.sub_energies(x[f], s["start"], m) for f, s, m in zip(frame, sigs, models)])
    starts = [s["start"] + ft4.SUB_SHIFTS[int(np.argmax(e))] for s, e in zip(sigs, en)]
    return np.array(models), bins, en, starts


def energy_gap(e):
    """(best - second best) / best of a case's 13 energies; 0 where every energy is 0"""
    s = np.sort(np.asarray(e, np.float64))[::-1]
    return (s[0] - s[1]) / s[0] if s[0] > 0 else 0.0


# ---- the residual: three noisy frames of four signals, in list order (f0 Hz, true start, snr dB, offset of the given start).  Frames 1
# and 2 hold a pair 12 and 20 Hz apart that overlaps in time: the second of a pair sees what the first left.  Frame 1 has a start
# before the frame, frame 2 a signal that runs past its end.
RESIDUAL = (((400.7, 4000, 5.0, -6), (900.2, 7000, -3.0, 11), (1500.9, 2000, 0.0, 3), (2200.4, 10000, -8.0, -14)),
            ((1000.3, 6000, 8.0, 9), (1012.0, 6700, -2.0, -5), (1800.5, 3000, 0.0, 18), (2600.1, -1500, 3.0, -2)),
            ((500.5, 33000, 6.0, -10), (1300.3, 5000, -6.0, 7), (1320.0, 5100, 4.0, -17), (3000.7, 8000, 0.0, 1)))
RESIDUAL_PAIRS = ((1, 0), (1, 1), (2, 1), (2, 2))      # (frame, signal) of the overlapping pairs


@functools.lru_cache(maxsize=None)
def residual_cases():
    """-> (audio int16 [3][90000], per frame the four signals as given to the decoder)"""
    ws = words(12, seed=3)
    frames, sigs = [], []
    for f, rows in enumerate(RESIDUAL):
        w4 = ws[4 * f:4 * f + 4]
        frames.append(ft4.frame_with_signals(10 + f, [(w, f0, start / ft4.FS, snr) for w, (f0, start, snr, _) in zip(w4, rows)]))
        sigs.append([sig(w, f0, start + off) for w, (f0, start, _, off) in zip(w4, rows)])
    return np.stack(frames), sigs


def twin_residual(frame_i16, sigs, starts):
    """the twin subtracting sigs at the given starts (refine 0) -> float64 [90000]"""
    x = np.asarray(frame_i16, np.float64).copy()
    ft4.subtract(x, [dict(s, start=int(t)) for s, t in zip(sigs, starts)], refine=0)
    return x


# ---- a contest message under a strong standard one (msg_types): 6 Hz and 0.1 s apart, 18 dB down
HIDDEN_TEXT = "TU; K1ABC W9XYZ 579 WI"


@functools.lru_cache(maxsize=None)
def hidden_frame():
    """-> (audio int16 [90000], the strong standard word, the contest word under it)"""
    strong, weak = synth.pack77("CQ", "K1ABC", "FN42"), synth.pack77_ext(HIDDEN_TEXT, None)
    return ft4.frame_with_signals(40, [(strong, 1000.0, 0.5, 10.0), (weak, 1006.0, 0.6, -8.0)]), strong, weak
