"""Shared inputs of tests/test_ddc_rat.py and tests/test_gpu_ddc_rat.py: the two FT8 channels of ddc_cases (a_i = frame(100 + i),
b_i = frame(200 + i)) placed in ONE stream at a rate that is no multiple of 12 kHz, by the FFT method of ddc_cases.recipe on 15 rate
points (661500 at 44100 Hz, 3750000 at 250 kHz: the bins are 1 / 15 Hz apart at any rate).  Built once, handed out unchanged."""
import numpy as np

import ddc_cases as cases

NSAMP = 180000
_recipes = {}


def offsets(rate, iq):
    """Dials of channels a and b: from the centre of an IQ stream (those of ddc_cases), absolute frequencies of a real one"""
    return cases.offsets(rate) if iq else (0.11 * rate, 0.31 * rate + 137.3)


def recipe(i, rate, iq):
    """-> (samples, [dial of each channel], [original 12 kHz frame of each channel]): IQ int16 [15 rate, 2] or real int16 [15 rate];
    a_i and b_i as USB channels at the two dials, a 9000-count tone at audio -1500 Hz of channel a and one at audio +7000 Hz of
    channel b.  The real stream is the real part of the IQ construction: each channel's analytic signal, mixed up to its dial."""
    key = (i, rate, iq)
    if key not in _recipes:
        n = 15 * rate
        chans = [(cases.frame(100 + i), offsets(rate, iq)[0], -1500.0), (cases.frame(200 + i), offsets(rate, iq)[1], 7000.0)]
        spec = np.zeros(n, np.complex128)
        for audio, f_off, _ in chans:
            cases._place(spec, audio, f_off)
        x = np.fft.ifft(spec) * n / NSAMP
        t = np.arange(n) / rate
        for _, f_off, f_tone in chans:
            x += 9000.0 * np.exp(2j * np.pi * (f_off + f_tone) * t)
        s = np.stack([np.rint(x.real), np.rint(x.imag)], axis=1) if iq else np.rint(x.real)
        assert (np.abs(s) >= 32767).mean() < 1e-4                 # (rounded to int16: a stray peak of the sum saturates)
        s = np.clip(s, -32768, 32767).astype(np.int16)
        s.setflags(write=False)
        _recipes[key] = (s, [c[1] for c in chans], [c[0] for c in chans])
    return _recipes[key]
