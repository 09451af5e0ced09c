"""Shared inputs of tests/test_ddc_stream.py and tests/test_gpu_ddc_stream.py: the frames of the live end-to-end test (six known
messages each), the two-cycle, two-channel IQ stream that carries them at 48 kHz, and the float64 twin's frame of every channel and
cycle.  Everything is built once and handed out unchanged."""
import numpy as np

import ddc_cases as cases
from pyft8_amd import ddc, synth

NSAMP = 180000
RATE = 48000
USED = (1, 2, 3)                          # the frames i whose control holds (tests/test_ddc_stream.py: test_live_inputs)
PLAN = ((1, 2), (3, 1))                   # cycle -> the frame on channel a, on channel b
BANDS = ("20m", "17m")
_msgs, _frames, _stream, _twin = {}, {}, [], {}


def messages(i):
    """Six random standard messages from the Philox key 0x5EED + i -> (their texts, their 77-bit words)"""
    if i not in _msgs:
        rng = np.random.Generator(np.random.Philox(key=0x5EED + i))
        m = [synth.random_message(rng) for _ in range(6)]
        _msgs[i] = (frozenset(" ".join(t) for t in m), [synth.pack77(*t) for t in m])
    return _msgs[i]


def frame(i):
    """The 12 kHz frame that carries messages(i) at 0 .. 8 dB"""
    if i not in _frames:
        _frames[i] = synth.frame_from_words(i, messages(i)[1], snr_range=(0, 8))
        _frames[i].setflags(write=False)
    return _frames[i]


def rotated(audio, phi):
    """The frame whose analytic signal is the frame's, rotated by phi rad: what a later cycle of a continuous mixer delivers"""
    spec = np.fft.fft(audio.astype(np.float64))
    spec[len(spec) // 2 + 1:] = 0.0
    spec[1:len(spec) // 2] *= 2.0
    return cases.to_frame(np.real(np.fft.ifft(spec) * np.exp(1j * phi)))


def offsets():
    return cases.offsets(RATE)


def stream():
    """IQ int16 [2 x 720000, 2] at 48 kHz: cycle c carries frame PLAN[c][0] as a USB channel at offsets()[0] and PLAN[c][1] at
    offsets()[1], each placed by its spectrum (ddc_cases._place).  The placement is periodic over 15 s: the concatenation has no jump."""
    if not _stream:
        n = NSAMP * RATE // 12000
        parts = []
        for ia, ib in PLAN:
            spec = np.zeros(n, np.complex128)
            for i, f_off in zip((ia, ib), offsets()):
                cases._place(spec, frame(i), f_off)
            parts.append(np.fft.ifft(spec) * n / NSAMP)
        x = np.concatenate(parts)
        iq = np.clip(np.stack([np.rint(x.real), np.rint(x.imag)], axis=1), -32768, 32767).astype(np.int16)
        iq.setflags(write=False)
        _stream.append(iq)
    return _stream[0]


def twin_frame(cycle, channel):
    """The float64 twin's frame of one channel and cycle of stream()"""
    key = (cycle, channel)
    if key not in _twin:
        y = ddc.reference_stream(stream(), ddc.IQ_I16, RATE, offsets()[channel], NSAMP * cycle, NSAMP * (cycle + 1))
        _twin[key] = cases.to_frame(y)
    return _twin[key]
