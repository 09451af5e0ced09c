"""Shared inputs of tests/test_ft4_live.py and tests/test_gpu_ft4_live.py (live FT4): the 7.5-s slots of the live
tests, the 48 kHz IQ streams that carry them, and the rows at which the float64 twin finds slot 0's six signals.  Everything is built
once and handed out unchanged."""
import numpy as np

import ddc_cases as cases
import ddc_stream_cases as live8
import ft4_sub_cases as sub4
from pyft8_amd import ft4

RATE = 48000
SLOT = ft4.NFRAME                          # 90000 outputs
T_SLOT = 7.5
EARLY = 72000                              # the default early pass: 6.0 s
SLOTS = (12, 17, None)                     # ft4.make_frame index of each slot of the FT4-only stream; None = the noise frame
# slot 0 (make_frame(12)): the search rows h0 of its six signals in the twin, on the slot zeroed from sample 72000 on -- the first four
# lie inside the early rule (144 h0 + 36 tt + 60624 <= 72000 needs h0 <= 78), the last two do not
ROWS_12 = (34, 40, 49, 59, 86, 102)
DIAL = 0.11 * RATE + 33.3                  # the one dial of the FT4-only stream
BAND = "40m"
T_FIRST = 7.5 * 1000                       # slot 1000 starts at output 0
_slots, _streams = {}, {}


def slot(i):
    """int16 [90000]: make_frame(i) with its six standard messages, or -- None -- noise alone"""
    if i not in _slots:
        _slots[i] = ft4.make_frame(i) if i is not None else ft4.frame_with_signals(7, [])
        _slots[i].setflags(write=False)
    return _slots[i]


def words(i):
    return [t["word"] for t in ft4.make_frame(i, return_truth=True)[1]]


def texts_by_start(i):
    """The texts of make_frame(i)'s six messages, by ascending start"""
    return [t["msg"] for t in sorted(ft4.make_frame(i, return_truth=True)[1], key=lambda t: t["t0"])]


def place(spec, audio, f_off):
    """The one-sided spectrum of a 12 kHz signal of any even length N (doubled except DC) at f_off Hz of the wide spectrum, whose length
    is N rate / 12000 (ddc_cases._place for any N); the placement is periodic over the signal"""
    n = len(audio)
    a = np.fft.rfft(audio.astype(np.float64))[:n // 2].copy()
    a[1:] *= 2.0
    spec[(int(round(f_off * n / 12000.0)) + np.arange(len(a))) % len(spec)] += a


def to_iq(spec, n_audio):
    x = np.fft.ifft(spec) * len(spec) / n_audio
    iq = np.clip(np.stack([np.rint(x.real), np.rint(x.imag)], axis=1), -32768, 32767).astype(np.int16)
    iq.setflags(write=False)
    return iq


def stream_ft4():
    """IQ int16 [3 x 360000, 2] at 48 kHz: the three slots of SLOTS joined, a USB channel at DIAL"""
    if "ft4" not in _streams:
        audio = np.concatenate([slot(i) for i in SLOTS])
        spec = np.zeros(len(audio) * RATE // 12000, np.complex128)
        place(spec, audio, DIAL)
        _streams["ft4"] = to_iq(spec, len(audio))
    return _streams["ft4"]


MIXED_FT8 = live8.PLAN[0][0]               # channel 0 of the mixed stream: that FT8 frame of tests/ddc_stream_cases.py
MIXED_FT4 = (12, 17)                       # channel 1: two FT4 slots
MIXED_BANDS = ("20m", "20m-ft4")


def stream_mixed():
    """IQ int16 [720000, 2] at 48 kHz, 15 s: channel 0 (ddc_stream_cases.offsets()[0]) one FT8 cycle, channel 1 (offsets()[1]) two FT4
    slots"""
    if "mixed" not in _streams:
        spec = np.zeros(live8.NSAMP * RATE // 12000, np.complex128)
        cases._place(spec, live8.frame(MIXED_FT8), live8.offsets()[0])
        place(spec, np.concatenate([slot(i) for i in MIXED_FT4]), live8.offsets()[1])
        _streams["mixed"] = to_iq(spec, live8.NSAMP)
    return _streams["mixed"]


CROWDED = sub4.CROWDED[1:]                # the slots of the crowded stream: 16 signals in 900 Hz each, where a second pass finds more
CROWDED_MAX_CANDS = 60                    # (tests/test_ft4_sub.py: the twin decodes 9 and 10 of the 16 in pass 1, 15 and 14 with a second)


def stream_crowded():
    """IQ int16 [720000, 2] at 48 kHz, 15 s: the two crowded slots of tests/ft4_sub_cases.py joined, a USB channel at DIAL"""
    if "crowded" not in _streams:
        audio = np.concatenate([sub4.crowded(i)[0] for i in CROWDED])
        spec = np.zeros(len(audio) * RATE // 12000, np.complex128)
        place(spec, audio, DIAL)
        _streams["crowded"] = to_iq(spec, len(audio))
    return _streams["crowded"]


def live_chunks(x):
    """The stream in chunks of 1920 and 1000 samples alternately -> (chunk, samples pushed once it is in)"""
    at, i = 0, 0
    while at < len(x):
        n = (1920, 1000)[i % 2]
        yield x[at:at + n], min(at + n, len(x))
        at, i = at + n, i + 1
