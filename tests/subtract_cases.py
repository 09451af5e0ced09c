"""Shared inputs of tests/test_subtract_oracle.py and tests/test_gpu_subtract.py: six frames with 13 signals to subtract, and the CPU
oracle's refine = 1 / refine = 2 results on them.  Everything is built once and handed out unchanged.

Frame E (edges): six signals, two so early that the coarse shifts reach start samples <= 0, one (t0 = 2.40 s) that cannot fit the
buffer (NSAMP - SUB_L = 28320 samples = 2.36 s; the per-shift guard of the scans decides where it locks), one at -4 dB.
Frame N (neighbours): four signals whose order matters, a later one sees the residual of the earlier ones: two co-channel
(3.1 Hz apart, 0.6 s apart) and two a tone spacing from each other.  The placement is the one first proposed; nothing had to be
moved: every pick of both oracles is unchanged under a +-0.01-count dither of the input (test_subtract_oracle.py).
Frame Z: noise, nothing to subtract.
Frames O0 .. O2: one signal each, origin outside the buffer: tsec = -0.5 and 20.0 (nothing may change), tsec = 0.0 (start sample 0:
only the positive shifts are valid).
The origin handed to subtract is the decoder's conventional one, (f0 - 1.9 Hz, t0 + 0.075 s) (ft8rx.hip, sub_shifts)."""
import numpy as np

from pyft8_amd import synth

NSAMP = 180000
SUB_L = 79 * 1920

_rng = np.random.default_rng(1)
WORDS = [synth.pack77(*synth.random_message(_rng)) for _ in range(10)]

E_SIGNALS = [(230.0, 0.02, 6), (700.3, 0.10, 3), (1500.0, 1.0, 8), (1900.2, 2.25, 4), (2650.0, 2.40, 6), (2790.0, 1.3, -4)]
N_SIGNALS = [(1000.0, 0.50, 6), (1003.1, 1.10, 3), (1050.0, 0.52, 0), (1043.75, 0.90, 8)]
E_UNFIT = 4                                              # the signal of frame E that runs off the end of the buffer
O_SIGNAL = (1002.75, 128.0 / 12000.0, 6)                 # word 0, where the tsec = 0.0 origin can reach it
O_ORIGINS = [(1000.0, -0.5), (1000.0, 20.0), (1000.0, 0.0)]
NAMES = ["E", "N", "Z", "O0", "O1", "O2"]
COUNTS = [6, 4, 0, 1, 1, 1]

_cache = {}


def _ro(a):
    a.setflags(write=False)
    return a


def _tones(word):
    return _ro(np.array(synth.tones79(word), np.uint8))


def frames():
    """int16 [6, 180000]: E, N, Z, O0, O1, O2."""
    if "frames" not in _cache:
        e = synth.frame_with_signals(7, [(WORDS[i], f, t, s) for i, (f, t, s) in enumerate(E_SIGNALS)])
        n = synth.frame_with_signals(8, [(WORDS[6 + i], f, t, s) for i, (f, t, s) in enumerate(N_SIGNALS)])
        z = synth.frame_with_signals(9, [])
        o = synth.frame_with_signals(10, [(0,) + O_SIGNAL])
        _cache["frames"] = _ro(np.stack([e, n, z, o, o, o]))
    return _cache["frames"]


def truth():
    """Per frame the (f0, t0) of each signal, None where the origin handed in has nothing to do with a signal."""
    return [[(f, t) for f, t, _ in E_SIGNALS], [(f, t) for f, t, _ in N_SIGNALS], [], [None], [None], [O_SIGNAL[:2]]]


def signals():
    """Per frame the list of (tones79, fHz, tsec) handed to subtract."""
    if "signals" not in _cache:
        e = [(_tones(WORDS[i]), f - 1.9, t + 0.075) for i, (f, t, _) in enumerate(E_SIGNALS)]
        n = [(_tones(WORDS[6 + i]), f - 1.9, t + 0.075) for i, (f, t, _) in enumerate(N_SIGNALS)]
        t0 = _tones(0)
        _cache["signals"] = [e, n, []] + [[(t0, f, t)] for f, t in O_ORIGINS]
    return _cache["signals"]


def rms(frame):
    """The RMS the 1e-4 bound refers to: of the frame's int16 audio."""
    return float(frames()[frame].astype(np.float64).std())


def run_oracle(mode, audio_f32, sigs):
    """The CPU oracle's refine = mode (1 or 2) over one frame's signals, in list order, in place on audio_f32
    -> [(fHz, tsec, subtracted)]."""
    import oracle as O
    out = []
    for tones, fHz, tsec in sigs:
        if mode == 2:
            done, f, t = O.refine2_subtract(audio_f32, tones, fHz, tsec, True)
        else:
            f, t = O.refine1(audio_f32, tones, fHz, tsec)
            done = O.subtract(audio_f32, tones, f, t)
        out.append((f, t, bool(done)))
    return out


def oracle_results(mode):
    """-> (per frame [(fHz, tsec, subtracted)], float32 residual [6, 180000]) of the oracle's refine = mode, computed once."""
    key = ("oracle", mode)
    if key not in _cache:
        wf = frames().astype(np.float32)
        picks = [run_oracle(mode, wf[f], signals()[f]) for f in range(len(COUNTS))]
        _cache[key] = (picks, _ro(wf))
    return _cache[key]


def grid_delta(a, b):
    """(start-sample difference, frequency difference in 1/64 Hz) of two origins (fHz, tsec)."""
    return int(12000.0 * a[1]) - int(12000.0 * b[1]), (a[0] - b[0]) * 64.0
