"""Crafted cases of the FT4 measured reports, shared by tests/test_ft4_report.py (the float64 twin,
pyft8_amd/ft4.py report) and tests/test_gpu_ft4_report.py (ft8rx_ft4_report against it).

A case is (name, frame, signal as given, n_have).  Every frame is a frame_with_signals frame with one planted signal unless its name
says otherwise; cases that share a frame are the same audio measured under other arguments.  Positions are the truth rounded to the
fine grid (36 samples, 2.6042 Hz) unless the case moves them."""
import functools

import numpy as np

from pyft8_amd import ft4, synth

# Bounds of the GPU test (tests/test_gpu_ft4_report.py): 4 x the worst value of the first run on an MI355X against the twin over
# CASES, rounded up to one digit (DESIGN.md section 19.9 has the measured values).  scores: max |P - P64| / max P64 over the 13 x 13
# map; on, off: relative; f_hz in Hz, t_sec in seconds, snr_db in dB.  Measured (the case it came from):
#   scores 1.981e-7 (noise only)   on 2.020e-7 (noise only)   off 1.513e-6 (start 48 samples off)
#   f_hz 7.837e-5 (start -0.3 s, 5730 Hz: half a unit of float32's last place there is 2.4e-4)   t_sec 4.959e-8 (start 48 samples off)
#   snr_db 7.666e-6 (fq 2 units off)
SCORE_BOUND = 8e-7
ON_BOUND = 9e-7
OFF_BOUND = 7e-6
F_BOUND = 4e-4
T_BOUND = 2e-7
SNR_BOUND = 4e-5
# a case is no near tie: the best P leads the runner-up by 100 x the score bound (relative to the best), and the quartile cell differs
# from both its neighbours in the sorted list
TIE_MARGIN = 100.0 * SCORE_BOUND

_RNG = np.random.Generator(np.random.Philox(key=ft4.SEED_BASE + 0x5290))
WORDS = [synth.pack77(*synth.random_message(_RNG)) for _ in range(12)]

# frame name -> (index, [(word, f0 Hz, t0 s, snr dB), ...], noise)
FRAMES = {
    "weak": (9000, [(WORDS[0], 1001.3, 0.5, -14.0)], True),
    "strong": (9001, [(WORDS[1], 1500.7, 1.4, 10.0)], True),                # ends at sample 77280: n_have 72000 leaves 94 valid
    "before": (9002, [(WORDS[2], 2200.4, -0.3, 0.0)], True),              # symbols 0 .. 6 lie before the frame: 97 valid
    "late": (9003, [(WORDS[3], 800.9, 5.0, 0.0)], True),                  # 90000 - 60000 = 52.08 symbols: 1 .. 51 are whole, 51 valid
    "too_late": (9004, [(WORDS[4], 1200.2, 6.0, 0.0)], True),             # 31.25 symbols: 1 .. 30 are whole, below 32: INVALID
    "low": (9005, [(WORDS[5], 15.0, 0.4, 0.0)], True),                    # fq 6: every cell below tone 0 is dropped
    "high": (9006, [(WORDS[6], 5900.0, 0.8, 0.0)], True),                 # fq 2266: every cell above tone 3 is dropped
    "pair": (9007, [(WORDS[7], 1400.0, 0.5, 3.0), (WORDS[8], 1460.0, 0.9, -3.0)], True),     # two overlapping signals 60 Hz apart
    "noise": (9008, [], True),
    "zero": (9009, [], False),
}


@functools.lru_cache(maxsize=None)
def frame(name):
    idx, sigs, noise = FRAMES[name]
    x = ft4.frame_with_signals(idx, sigs, noise=noise)
    x.setflags(write=False)
    return x


def given(word, f0, t0, d_start=0, d_fq=0):
    """the signal dict at the truth rounded to the fine grid, moved by d_start samples and d_fq units of 2.6042 Hz"""
    s0 = ft4.DT_STEP * int(np.rint(t0 * ft4.FS / ft4.DT_STEP)) + d_start
    fq = int(np.rint(f0 / ft4.DF_HZ)) + d_fq
    return dict(start=s0, fq=fq, tones=ft4.tones105(word), word=word)


def _planted(name, k=0, **kw):
    w, f0, t0, _ = FRAMES[name][1][k]
    return given(w, f0, t0, **kw)


# (name, frame, signal, n_have)
CASES = [
    ("interior -14 dB", "weak", _planted("weak"), 90000),
    ("interior +10 dB", "strong", _planted("strong"), 90000),
    ("start -0.3 s", "before", _planted("before"), 90000),
    ("start 5.0 s", "late", _planted("late"), 90000),
    ("start 6.0 s", "too_late", _planted("too_late"), 90000),
    ("f0 15 Hz", "low", _planted("low"), 90000),
    ("f0 5900 Hz", "high", _planted("high"), 90000),
    ("start 48 samples off", "strong", _planted("strong", d_start=48), 90000),
    ("fq 2 units off", "strong", _planted("strong", d_fq=2), 90000),
    ("start and fq off", "strong", _planted("strong", d_start=-48, d_fq=2), 90000),
    ("n_have 72000", "strong", _planted("strong"), 72000),
    ("pair, the stronger", "pair", _planted("pair", 0), 90000),
    ("pair, the weaker", "pair", _planted("pair", 1), 90000),
    ("noise only", "noise", given(WORDS[9], 1200.0, 0.5), 90000),
    ("all zero", "zero", given(WORDS[10], 400.0 * ft4.DF_HZ, 1008 / 12000.0), 90000),
]
# what each case must show (flags of the twin), by name
WANT_FLAGS = {
    "start 6.0 s": ft4.RP_MEASURED | ft4.RP_INVALID,
    "start 48 samples off": ft4.RP_MEASURED | ft4.RP_EDGE_T,
    "fq 2 units off": ft4.RP_MEASURED | ft4.RP_EDGE_F,
    "start and fq off": ft4.RP_MEASURED | ft4.RP_EDGE_T | ft4.RP_EDGE_F,
    "all zero": ft4.RP_MEASURED | ft4.RP_EDGE_T | ft4.RP_EDGE_F,
}
WANT_VALID = {"start -0.3 s": 97, "start 5.0 s": 51, "start 6.0 s": 30, "n_have 72000": 94}


@functools.lru_cache(maxsize=None)
def twin(i):
    """ft4.report of case i (full: with the sorted cells); computed once, shared by both test files"""
    _, fr, sig, n_have = CASES[i]
    return ft4.report(frame(fr), sig, n_have=n_have, full=True)


def subsig_array(sigs):
    from pyft8_amd import _lib
    a = np.zeros(len(sigs), _lib.FT4_SUBSIG_DTYPE)
    for i, s in enumerate(sigs):
        a[i]["start"], a[i]["fq"], a[i]["tones"] = s["start"], s["fq"], np.asarray(s["tones"], np.uint8)
    return a


def calls():
    """The cases packed into calls of the smallest batch shape, 3 frames x 5 signals with counts (5, 0, 3): the cases of one n_have,
    frame by frame; a call takes a frame with up to five cases, an idle frame, and a frame with up to three -> [(n_have, audio
    [3][90000], sigs [3][5], counts, {(row, slot): case index})]"""
    out = []
    for n_have in sorted({c[3] for c in CASES}):
        by_frame = {}
        for i, c in enumerate(CASES):
            if c[3] == n_have:
                by_frame.setdefault(c[1], []).append(i)
        groups = []
        for fr, idx in by_frame.items():
            while idx:
                groups.append((fr, idx[:3])); idx = idx[3:]
        groups += [("noise", [])] * (len(groups) % 2)
        for (fa, ia), (fb, ib) in zip(groups[0::2], groups[1::2]):
            if len(ib) > len(ia):
                (fa, ia), (fb, ib) = (fb, ib), (fa, ia)
            from pyft8_amd import _lib
            sigs = np.zeros((3, 5), _lib.FT4_SUBSIG_DTYPE)
            sigs[0, :len(ia)] = subsig_array([CASES[i][2] for i in ia])
            sigs[2, :len(ib)] = subsig_array([CASES[i][2] for i in ib])
            where = {(0, k): i for k, i in enumerate(ia)}
            where.update({(2, k): i for k, i in enumerate(ib)})
            out.append((n_have, np.stack([frame(fa), frame("noise"), frame(fb)]), sigs, np.array([len(ia), 0, len(ib)], np.int32), where))
    return out


def batch():
    """The byte-for-byte fixture: 3 frames, max_sigs 5, counts (5, 0, 3) -- the strong frame under five arguments, an idle frame, the
    pair's frame under three"""
    from pyft8_amd import _lib
    sigs = np.zeros((3, 5), _lib.FT4_SUBSIG_DTYPE)
    sigs[0] = subsig_array([_planted("strong"), _planted("strong", d_start=48), _planted("strong", d_fq=2), _planted("strong", d_start=-12, d_fq=1),
                            _planted("strong", d_start=-48, d_fq=2)])
    sigs[2, :3] = subsig_array([_planted("pair", 0), _planted("pair", 1), given(WORDS[11], 2000.0, 0.3)])
    return np.stack([frame("strong"), frame("noise"), frame("pair")]), sigs, np.array([5, 0, 3], np.int32)


# ----------------------------------------------------------------------------- the accuracy recipe and its bounds (section 14's, for FT8)
RECIPE = dict(n_signals=8, snr_range=(-14, 15), min_sep_hz=250, return_truth=True)
TWIN_FRAMES = range(0, 16)             # through the twin on the CPU, positions from decode_twin
GPU_FRAMES = range(16, 80)             # through the GPU


def recipe_frame(i):
    """ft4.make_frame(i, **RECIPE), or None at the indices where eight carriers 250 Hz apart do not fit make_frame's default band
    (0, 7, 33, 35 and 57 of 0 .. 79: the generator gives up, and the recipe has no frame there)"""
    try:
        return ft4.make_frame(i, **RECIPE)
    except ValueError:
        return None


def error_stats(rows):
    """rows of (truth snr, snr error dB, frequency error Hz, time error ms) -> the figures the bounds are set on"""
    e = np.asarray(rows, np.float64).reshape(-1, 4)
    lo, hi = e[e[:, 0] <= 0.0], e[e[:, 0] > 0.0]
    rms = lambda v: float(np.sqrt((v ** 2).mean())) if len(v) else 0.0
    mean = lambda v: float(v.mean()) if len(v) else 0.0
    return dict(n=len(e), n_low=len(lo), n_high=len(hi),
                snr_low_mean=mean(lo[:, 1]), snr_low_rms=rms(lo[:, 1]), snr_high_mean=mean(hi[:, 1]),
                snr_high_worst=float(np.abs(hi[:, 1]).max()) if len(hi) else 0.0,
                f_mean=mean(e[:, 2]), f_rms=rms(e[:, 2]), t_mean=mean(e[:, 3]), t_std=float(e[:, 3].std()) if len(e) else 0.0)


def check_bounds(s):
    """the bounds of the issue: section 14's for FT8"""
    assert abs(s["snr_low_mean"]) <= 1.0 and s["snr_low_rms"] <= 1.5, s
    assert -3.0 <= s["snr_high_mean"] <= 1.0 and s["snr_high_worst"] <= 6.0, s
    assert abs(s["f_mean"]) <= 0.1 and s["f_rms"] <= 0.25, s
    assert abs(s["t_mean"]) <= 1.0 and s["t_std"] <= 1.0, s
