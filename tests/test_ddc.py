"""The down-converter's definition on the CPU (no GPU needed): the taps the library hands out, the response of
the float64 twin (pyft8_amd/ddc.py: reference) to tones, two FT8 channels carried in one IQ stream through the twin and the CPU
oracle, and the wav reader."""
import wave

import numpy as np
import pytest

import ddc_cases as cases
from pyft8_amd import _lib, ddc

DS = (1, 2, 4, 8, 16)
N1 = {4: 17, 8: 31, 16: 61}


def test_tap_counts_symmetry_and_gain():
    for D in DS:
        rate = 12000 * D
        h1, h2 = ddc.taps(rate, 1), ddc.taps(rate, 2)
        assert len(h1) == N1.get(D, 0) and len(h2) == (143 if D == 1 else 283)
        for h in (h1, h2):
            if len(h):
                assert h.dtype == np.float32 and np.array_equal(h, h[::-1])
                assert abs(h.astype(np.float64).sum() - 1.0) <= len(h) * 2.0 ** -24          # unit DC gain within float32 rounding
                assert h[len(h) // 2] == h.max() > 0
    L = _lib.lib()
    for rate in (0, 8000, 44100, 36000, 384000, -48000):
        assert L.ft8rx_ddc_taps(rate, 1, None, 0) == -1 and L.ft8rx_ddc_taps(rate, 2, None, 0) == -1
        with pytest.raises(_lib.Ft8rxError, match="rate"):
            ddc.taps(rate, 2)
    assert L.ft8rx_ddc_taps(48000, 3, None, 0) == -1 and L.ft8rx_ddc_taps(48000, 0, None, 0) == -1
    assert L.ft8rx_ddc_taps(48000, 2, None, 0) == 283 and L.ft8rx_ddc_taps(24000, 1, None, 0) == 0          # the count alone
    part = np.full(8, -1.0, np.float32)
    assert L.ft8rx_ddc_taps(48000, 1, part.ctypes.data, 5) == 17 and np.array_equal(part[:5], ddc.taps(48000, 1)[:5]) and (part[5:] == -1).all()


T_IN = 1.0                      # seconds of tone: long against the filters (283 taps at 24 kHz = 12 ms)
M_LO, M_HI = 600, 11400         # the outputs measured: inside the tone, clear of both filter transients


def tone_out(D, kind, f_dial, f_in):
    """The twin's output for a unit tone at f_in Hz from the stream's centre (complex for IQ kinds, a cosine for real ones)."""
    rate = 12000 * D
    t = np.arange(int(T_IN * rate)) / rate
    x = np.exp(2j * np.pi * f_in * t) if ddc.is_iq(kind) else np.cos(2 * np.pi * f_in * t)
    y, f_mixed = ddc.reference(x, kind, rate, f_dial)
    assert abs(f_mixed - f_dial) <= 0.5 * rate / 2.0 ** 32 * (1 + 1e-9)
    return y[M_LO:M_HI]


def level_db(y):
    return 10.0 * np.log10(2.0 * np.mean(y ** 2) + 1e-300)          # 0 dB = a unit sinusoid


def fit(y, f_audio):
    """Least-squares sinusoid at f_audio: (amplitude, frequency offset in Hz read off the phase drift between the two halves)."""
    m = np.arange(M_LO, M_HI)
    e = np.exp(-2j * np.pi * f_audio * m / 12000.0)
    half = len(m) // 2
    basis = lambda s: np.stack([e[s].real, e[s].imag], axis=1)
    ph = []
    for s in (slice(0, half), slice(half, 2 * half)):
        c = np.linalg.lstsq(basis(s), y[s], rcond=None)[0]
        ph.append(np.angle(c[0] + 1j * c[1]))
    c = np.linalg.lstsq(basis(slice(None)), y, rcond=None)[0]
    dphi = (ph[1] - ph[0] + np.pi) % (2 * np.pi) - np.pi
    return float(np.hypot(*c)), float(dphi / (2 * np.pi) * 12000.0 / half)


@pytest.mark.parametrize("D", DS)
def test_response(D):
    rate = 12000 * D
    f_dial = -0.31 * rate
    kind = ddc.IQ_F32
    res = rate / 2.0 ** 32
    for fa in (200.0, 517.3, 1500.0, 3000.0, 4400.0, 5800.0):                          # the USB passband
        y = tone_out(D, kind, f_dial, f_dial + fa)
        amp, df = fit(y, fa)
        print(f"D={D} audio {fa:7.1f} Hz: {20 * np.log10(amp):+.4f} dB, frequency off by {df:+.2e} Hz (resolution {res:.2e})")
        assert abs(20 * np.log10(amp)) <= 0.05
        assert abs(df) <= res
    stop = [-200.0, -700.0, -3000.0, -6000.0, 6200.0, 6700.0, 9000.0, 11999.0]
    stop += [0.5 * rate - 3000.0 - 1.0, -0.5 * rate - 3000.0 + 1.0]                    # the stream's edges (baseband +-rate/2)
    for k in range(1, D // 2 + 1):                                                     # what stage 1 folds onto the passband: k 24 kHz +- 3 kHz
        for s in (-1, 1):
            stop += [3000.0 + s * k * 24000.0 + d for d in (-3000.0, -1400.0, 0.0, 2800.0)]
    worst = -999.0
    for fa in stop:
        fb = (fa - 3000.0 + 0.5 * rate) % rate - 0.5 * rate                            # the same tone inside the stream (the spectrum wraps)
        if -3200.0 < fb < 3200.0:
            continue                                                                   # folded into the passband or its skirts by the wrap itself
        lv = level_db(tone_out(D, kind, f_dial, f_dial + fa))
        worst = max(worst, lv)
        assert lv <= -70.0, (D, fa, lv)
    print(f"D={D}: worst stopband tone {worst:.1f} dB")


@pytest.mark.parametrize("D,kind,f_dial", [(1, ddc.REAL_F32, 0.0), (2, ddc.REAL_I16, 3500.0), (4, ddc.REAL_I16, 0.0), (4, ddc.REAL_F32, 14000.0),
                                           (16, ddc.REAL_F32, 70000.0)])
def test_real_kinds_have_unit_gain(D, kind, f_dial):
    for fa in (300.0, 2500.0, 5700.0):
        amp, df = fit(tone_out(D, kind, f_dial, f_dial + fa), fa)
        assert abs(20 * np.log10(amp)) <= 0.05 and abs(df) <= 12000 * D / 2.0 ** 32


@pytest.mark.parametrize("i,D", [(0, 4), (1, 4), (2, 4), (0, 16), (0, 1), (0, 2)])
def test_two_channels_through_twin_and_oracle(i, D):
    """a_i and b_i in one IQ int16 stream, a strong tone next to each: the oracle decodes from the twin's frame what it decodes from
    the original frame (D = 1: channel a alone)."""
    iq, offs, originals = cases.recipe(i, D, only_a=(D == 1))
    for j, (f_off, original) in enumerate(zip(offs, originals)):
        y, _ = ddc.reference(iq, ddc.IQ_I16, 12000 * D, f_off)
        got, want = cases.oracle_texts(cases.to_frame(y)), cases.oracle_texts(original)
        print(f"i={i} D={D} channel {'ab'[j]}: {len(got)} messages, original frame {len(want)}")
        assert got == want and len(want) >= 5


def test_iq_from_wav(tmp_path):
    rng = np.random.default_rng(5)
    x = rng.integers(-32768, 32768, size=(4801, 2)).astype(np.int16)

    def write(name, data, channels, rate, width=2):
        p = str(tmp_path / name)
        with wave.open(p, "wb") as w:
            w.setnchannels(channels); w.setsampwidth(width); w.setframerate(rate)
            w.writeframes(data.tobytes())
        return p
    s, kind, rate = ddc.iq_from_wav(write("iq.wav", x, 2, 96000))
    assert kind == ddc.IQ_I16 and rate == 96000 and s.dtype == np.int16 and np.array_equal(s, x)          # I = left, Q = right
    s, kind, rate = ddc.iq_from_wav(write("mono.wav", x[:, 0].copy(), 1, 48000))
    assert kind == ddc.REAL_I16 and rate == 48000 and np.array_equal(s, x[:, 0])
    arr, n_streams, n = ddc.pack(s, kind)
    assert (n_streams, n) == (1, 4801) and arr.dtype == np.int16
    arr, n_streams, n = ddc.pack(x, ddc.IQ_I16)
    assert arr.shape == (1, 4801, 2)
    for args, word in ((("r.wav", x, 2, 44100), "rate"), (("m12.wav", x[:, 0].copy(), 1, 12000), "rate"),
                       (("w.wav", x.astype(np.uint8), 2, 48000, 1), "sample width"), (("c.wav", np.zeros((10, 3), np.int16), 3, 48000), "channels")):
        with pytest.raises(_lib.Ft8rxError, match=word):
            ddc.iq_from_wav(write(*args))
    # the 12 kHz frame reader keeps its refusal
    from pyft8_amd.receiver import frames_from_wav
    with pytest.raises(_lib.Ft8rxError, match="need mono 16-bit 12000 Hz"):
        frames_from_wav(write("iq2.wav", x, 2, 96000))


def test_twin_refusals_name_the_argument():
    x = np.zeros(100)
    for args, word in (((x, 9, 48000, 0.0), "kind"), ((x, ddc.REAL_F32, 44100, 0.0), "rate"), ((x, ddc.REAL_I16, 12000, 0.0), "real int16"),
                       ((x, ddc.REAL_F32, 48000, 24000.0), "f_dial_hz"), ((np.zeros(180000 * 2 + 1), ddc.REAL_F32, 24000, 0.0), "samples"),
                       ((x + 0j, ddc.REAL_F32, 48000, 0.0), "x"), ((x, ddc.IQ_F32, 48000, 0.0), "x")):
        with pytest.raises(_lib.Ft8rxError, match=word):
            ddc.reference(*args)
