"""Shared inputs of tests/test_ddc.py and tests/test_gpu_ddc.py: the two-channel IQ recipes of the down-converter's end-to-end tests,
and the oracle's message set of a 12 kHz frame.  Everything is built once and handed out unchanged."""
import numpy as np

from pyft8_amd import _lib, synth

NSAMP = 180000
_frames, _recipes, _oracle = {}, {}, {}


def frame(index):
    """a_i = frame(100 + i), b_i = frame(200 + i): ten signals at -6 .. +6 dB between 250 and 2800 Hz."""
    if index not in _frames:
        _frames[index] = synth.make_frame(index, n_signals=10, snr_range=(-6, 6), freq_range=(250, 2800))
        _frames[index].setflags(write=False)
    return _frames[index]


def offsets(rate):
    """Dial offsets of channels a and b from the stream's centre."""
    return -0.31 * rate, 0.22 * rate + 137.3


def _place(spec, audio, f_off):
    """The frame's one-sided spectrum (rfft bins 0 .. 89999, doubled except DC) at bin round(15 f_off) of the wide spectrum (wrapping)."""
    a = np.fft.rfft(audio.astype(np.float64))[:NSAMP // 2].copy()
    a[1:] *= 2.0
    idx = (int(round(15.0 * f_off)) + np.arange(len(a))) % len(spec)
    spec[idx] += a


def recipe(i, D, only_a=False):
    """-> (IQ int16 [180000 D, 2], [f_off of each channel], [original 12 kHz frame of each channel]) at rate 12000 D: a_i and b_i as
    USB channels at the two offsets, a 9000-count complex tone at audio -1500 Hz of channel a and one at audio +7000 Hz of channel b
    (only_a: channel a and its tone alone)."""
    key = (i, D, only_a)
    if key not in _recipes:
        rate, n = 12000 * D, NSAMP * D
        fa, fb = offsets(rate)
        chans = [(frame(100 + i), fa, -1500.0)] + ([] if only_a else [(frame(200 + i), fb, 7000.0)])
        spec = np.zeros(n, np.complex128)
        for audio, f_off, _ in chans:
            _place(spec, audio, f_off)
        x = np.fft.ifft(spec) * n / NSAMP
        t = np.arange(n) / rate
        for _, f_off, f_tone in chans:
            x += 9000.0 * np.exp(2j * np.pi * (f_off + f_tone) * t)
        iq = np.clip(np.stack([np.rint(x.real), np.rint(x.imag)], axis=1), -32768, 32767)
        assert (np.abs(iq) >= 32767).mean() < 1e-4                # (rounded to int16: a stray peak of the sum saturates)
        iq = iq.astype(np.int16)
        iq.setflags(write=False)
        _recipes[key] = (iq, [c[1] for c in chans], [c[0] for c in chans])
    return _recipes[key]


def oracle_texts(audio_i16):
    """The CPU oracle's message set of one 12 kHz frame (cached by content)."""
    import oracle as O
    audio_i16 = np.ascontiguousarray(audio_i16, np.int16)
    key = hash(audio_i16.tobytes())
    if key not in _oracle:
        r = O.decode_frame(audio_i16, O.default_config(**_lib.fft_plans()))
        _oracle[key] = frozenset(" ".join(m["msg_tuple"]) for m in r["msgs"])
    return _oracle[key]


def to_frame(y):
    """rint and saturation: the frame of a float output."""
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16)
