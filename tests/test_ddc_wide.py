"""The wide pre-decimator on the CPU (no GPU needed): plans and taps from the library against a numpy design of
the same recipe, the response of the float64 twin (pyft8_amd/ddc_wide.py) to unit tones, the twin's identities, two FT8 channels in one
240 kHz stream through twin and oracle, and the index arithmetic (csrc/ddc_wide_ring.hpp) under the host sanitizers.

Measured with the twin (printed by test_response), dial 0.137 rate, pre-filter designed at A = 85 dB:
  240 kHz:  audio 200 .. 5800 Hz within 0.0011 dB; worst stopband tone -79.8 dB; worst image of the 48 kHz stream -85.5 dB
  2.4 MHz:  audio 200 .. 5800 Hz within 0.0018 dB; worst stopband tone -79.8 dB; worst image of the 96 kHz stream -83.2 dB"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ddc_cases as cases
from conftest import ROOT
from pyft8_amd import _lib, ddc
from pyft8_amd import ddc_wide as dw

NSAMP = 180000
PLANS = {240000: (48000, 5, 33), 384000: (192000, 2, 13), 768000: (192000, 4, 25), 2400000: (96000, 25, 145),
         64800000: (96000, 675, 3883), 129600000: (192000, 675, 3749)}
REFUSED = (250000, 2048000, 192000, 144000, 129648000)


def kaiser_design(f_pass, f_stop, A, fs):
    """The project's recipe in numpy: Kaiser estimate of the length, made odd; cutoff half way; unit DC gain"""
    N = int(np.ceil((A - 7.95) / (2.285 * 2.0 * np.pi * (f_stop - f_pass) / fs))) + 1
    N += 1 - N % 2
    x = np.arange(N) - (N - 1) / 2.0
    h = 2.0 * (f_pass + f_stop) / (2.0 * fs) * np.sinc(2.0 * (f_pass + f_stop) / (2.0 * fs) * x) * np.kaiser(N, 0.1102 * (A - 8.7))
    return h / h.sum()


def test_plans_and_taps():
    L = _lib.lib()
    for rate, (mid, r0, n) in PLANS.items():
        assert dw.plan(rate) == (mid, r0) and dw.accepts(rate)
        h = dw.taps(rate)
        want = kaiser_design(3200.0, mid - 3200.0, 85.0, float(rate))
        assert len(h) == n == len(want) and h.dtype == np.float32
        assert np.abs(h.astype(np.float64) - want).max() <= 1e-6 * want.max()
        assert np.array_equal(h, h[::-1]) and h[n // 2] == h.max() > 0
        assert abs(h.astype(np.float64).sum() - 1.0) <= n * 2.0 ** -24          # unit DC gain within float32 rounding
        assert L.ft8rx_ddc_wide_taps(rate, None, 0) == n                        # the count alone
    for rate in REFUSED + (0, -240000, 48000 * 1351):
        assert not dw.accepts(rate) and L.ft8rx_ddc_wide_taps(rate, None, 0) == -1 and L.ft8rx_ddc_wide_plan(rate, None, None) == -1
        with pytest.raises(_lib.Ft8rxError, match="rate"):
            dw.plan(rate)
        with pytest.raises(_lib.Ft8rxError, match="rate"):
            dw.taps(rate)
    assert dw.plan(48000 * 1349) == (48000, 1349) and len(dw.taps(48000 * 1349)) <= 8448      # the longest filter the kernel takes
    part = np.full(8, -1.0, np.float32)
    assert L.ft8rx_ddc_wide_taps(240000, part.ctypes.data, 5) == 33 and np.array_equal(part[:5], dw.taps(240000)[:5]) and (part[5:] == -1).all()
    # ddc.py keeps its refusals
    for rate in PLANS:
        with pytest.raises(_lib.Ft8rxError, match="rate"):
            ddc.decimation(rate)


def test_frequency_words_kinds_and_pack():
    for rate in PLANS:
        mid = PLANS[rate][0]
        for f in (-0.5 * rate, -0.5 * rate + 400.0, 0.0, 0.137 * rate, 0.5 * rate - 700.0, 0.5 * rate - 3000.0):
            w0, f0, d, fm = dw.frequency_words(rate, f)
            assert 0 <= w0 < 2 ** 32 and -0.5 * rate <= f0 < 0.5 * rate and -0.5 * rate <= fm < 0.5 * rate
            assert abs(d + 3000.0) <= 0.5 * rate / 2.0 ** 32 * (1 + 1e-9)                       # the wanted audio sits at the centre
            off = (fm - f + 0.5 * rate) % rate - 0.5 * rate
            assert abs(off) <= 0.5 * mid / 2.0 ** 32 * (1 + 1e-6)                               # what is left is the stage behind's resolution
    z16, zu8, zi8 = np.zeros((4, 2), np.int16), np.zeros((4, 2), np.uint8), np.zeros((4, 2), np.int8)
    assert [dw.kind_of(a, True) for a in (z16, zu8, zi8)] == [dw.IQ_I16, dw.IQ_U8, dw.IQ_I8] and dw.kind_of(z16[:, 0], False) == dw.REAL_I16
    for a, iq, word in ((np.zeros(4, np.float32), False, "float32"), (np.zeros(4, np.complex64), True, "complex64"), (zu8[:, 0], False, "uint8")):
        with pytest.raises(_lib.Ft8rxError, match=word):
            dw.kind_of(a, iq)
    assert dw.pack(zu8, dw.IQ_U8)[1] == 4 and dw.pack([1, -2, 3], dw.REAL_I16)[0].dtype == np.int16
    for a, kind, word in ((z16, dw.REAL_I16, "shape"), (z16[:, 0], dw.IQ_I16, "shape"), (np.array([[300, 0]]), dw.IQ_I8, "int8 range"),
                          (np.zeros((2, 4, 2), np.int16), dw.IQ_I16, "ONE stream"), (z16, 3, "kind")):
        with pytest.raises(_lib.Ft8rxError, match=word):
            dw.pack(a, kind)
    x = np.array([[0, 255], [128, 127]], np.uint8)
    assert np.array_equal(dw.sample_values(x, dw.IQ_U8), [-32640 + 32640j, 128 - 128j])
    assert np.array_equal(dw.sample_values(np.array([[-128, 127]], np.int8), dw.IQ_I8), [-32768 + 32512j])


# ---- the response of the twin to unit tones
T_IN = 1.0                      # seconds of tone: long against every filter of the chain
M_LO, M_HI = 600, 11400         # the outputs measured: inside the tone, clear of the transients


def tone_out(rate, f_dial, f_in):
    x = np.exp(2j * np.pi * f_in * (np.arange(int(T_IN * rate)) / rate))
    y, f_mixed = dw.reference(x, dw.IQ_I16, rate, f_dial)
    assert abs(f_mixed - f_dial) <= 0.5 * rate / 2.0 ** 32 * (1 + 1e-9) + 0.5 * dw.plan(rate)[0] / 2.0 ** 32
    return y[M_LO:M_HI]


def level_db(y):
    return 10.0 * np.log10(2.0 * np.mean(y ** 2) + 1e-300)          # 0 dB = a unit sinusoid


def amplitude(y, f_audio):
    e = np.exp(-2j * np.pi * f_audio * np.arange(M_LO, M_HI) / 12000.0)
    c = np.linalg.lstsq(np.stack([e.real, e.imag], axis=1), y, rcond=None)[0]
    return float(np.hypot(*c))


@pytest.mark.parametrize("rate", [240000, 2400000])
def test_response(rate):
    """The standing promise of ft8rx_ddc with the pre-stage in front: audio 200 .. 5800 Hz within +-0.003 dB; audio <= -200 Hz and
    >= 6200 Hz, and the images of the intermediate rate, at least 74 dB down"""
    mid = dw.plan(rate)[0]
    f_dial = 0.137 * rate
    worst_pass = 0.0
    for fa in (200.0, 517.3, 1500.0, 3000.0, 4400.0, 5800.0):
        db = 20 * np.log10(amplitude(tone_out(rate, f_dial, f_dial + fa), fa))
        print(f"rate {rate} audio {fa:7.1f} Hz: {db:+.5f} dB")
        worst_pass = max(worst_pass, abs(db))
    worst_stop, worst_image = -999.0, -999.0
    for fa in (-200.0, -700.0, -3000.0, -6000.0, 6200.0, 6700.0, 9000.0, 11999.0, 0.5 * mid + 3000.0, 0.5 * rate + 2999.0):
        worst_stop = max(worst_stop, level_db(tone_out(rate, f_dial, f_dial + fa)))
    for k in (-2, -1, 1, 2):
        for a in (200.0, 3000.0, 5800.0):
            lv = level_db(tone_out(rate, f_dial, f_dial + a + k * mid))
            print(f"rate {rate} image {k:+d} x {mid} of audio {a:6.1f} Hz: {lv:.2f} dB")
            worst_image = max(worst_image, lv)
    print(f"rate {rate}: passband within {worst_pass:.5f} dB, worst stopband tone {worst_stop:.2f} dB, worst image {worst_image:.2f} dB")
    assert worst_pass <= 0.003
    assert worst_stop <= -74.0 and worst_image <= -74.0


# ---- twin identities
def random_iq(n, key, dtype):
    rng = np.random.Generator(np.random.Philox(key=0xD1DE + key))
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max + 1, size=(n, 2), dtype=np.int64).astype(dtype)


def test_eight_bit_kinds_are_the_int16_twin_on_the_converted_samples():
    rate, f = 240000, 0.11 * 240000
    u = random_iq(24000, 1, np.uint8)
    s = random_iq(24000, 2, np.int8)
    as16_u = (256 * u.astype(np.int32) - 32640).astype(np.int16)
    as16_s = (256 * s.astype(np.int32)).astype(np.int16)
    for x8, kind, x16 in ((u, dw.IQ_U8, as16_u), (s, dw.IQ_I8, as16_s)):
        a = dw.reference_stream(x8, kind, rate, f, 0, 1100)
        b = dw.reference_stream(x16, dw.IQ_I16, rate, f, 0, 1100)
        assert np.abs(a).max() > 1000 and np.abs(a - b).max() <= 1e-9
        assert np.array_equal(dw.reference_mid(x8, kind, rate, f, 0, 500), dw.reference_mid(x16, dw.IQ_I16, rate, f, 0, 500))
    # the real kind: twice the real part of the same samples taken as IQ with Q = 0
    r = random_iq(24000, 3, np.int16)
    r[:, 1] = 0
    a = dw.reference_mid(r[:, 0].copy(), dw.REAL_I16, rate, f, 10, 300)
    assert np.abs(a - 2.0 * dw.reference_mid(r, dw.IQ_I16, rate, f, 10, 300)).max() <= 1e-9 * np.abs(a).max()


@pytest.mark.parametrize("rate,kind", [(240000, dw.IQ_I16), (768000, dw.IQ_U8), (2400000, dw.REAL_I16)])
def test_stream_twin_from_the_origin_is_the_one_shot(rate, kind):
    n = rate // 4
    x = random_iq(n, rate // 1000, dw._DTYPE[kind])
    x = x[:, 0].copy() if kind == dw.REAL_I16 else x
    for f in (-0.5 * rate + 400.0, 0.11 * rate, 0.5 * rate - 700.0):
        y, fm = dw.reference(x, kind, rate, f, gain=0.7)
        ys = dw.reference_stream(x, kind, rate, f, 0, 3200, gain=0.7)
        assert np.abs(y[:3200]).max() > 1000 and np.abs(ys - y[:3200]).max() <= 1e-9
        assert fm == dw.frequency_words(rate, f)[3]
    assert not dw.reference(x[:0], kind, rate, 0.0)[0].any()                      # no samples: a frame of zeros


def test_origin_shift_and_the_phase_rule_across_2_to_the_32():
    """The same samples as a stream that begins s = k 1008 x 20 later (240 kHz), asked for the outputs shifted by s / 20.  The shifted
    stream's first mixer is ahead by phi0 = (w0 s mod 2^32) / 2^32 cycles and the second, which begins s / R0 intermediate samples later,
    by phi1 = (w1 s / R0 mod 2^32) / 2^32; i^m is unchanged because s / 20 is a multiple of 4.  So the shifted stream of
    x e^{+2 pi i (phi0 + phi1)} gives the values of x.  k = 213041 puts the shifted stream across n = 2^32."""
    rate, grid = 240000, 1008 * 20
    mid, R0 = dw.plan(rate)
    x = random_iq(100000, 7, np.int16).astype(np.float64)
    x = x[:, 0] + 1j * x[:, 1]
    lo, hi = -100, 4000
    for k in (5, 213041):
        s = k * grid
        assert k == 5 or s < 2 ** 32 < s + len(x)
        for f in (0.22 * rate + 137.3, -0.5 * rate + 400.0):
            w0, _, d, _ = dw.frequency_words(rate, f)
            w1, _ = ddc.frequency_word(mid, d)
            phi = ((w0 * s) % 2 ** 32 + (w1 * (s // R0)) % 2 ** 32) / 2.0 ** 32
            y = dw.reference_stream(x, dw.IQ_I16, rate, f, lo, hi)
            ys = dw.reference_stream(x * np.exp(2j * np.pi * phi), dw.IQ_I16, rate, f, lo + s // 20, hi + s // 20, n_origin=s)
            assert np.abs(y).max() > 1000 and np.abs(ys - y).max() <= 1e-9 * 32768
    with pytest.raises(_lib.Ft8rxError, match="n_origin"):
        dw.reference_stream(x, dw.IQ_I16, rate, 0.0, 0, 10, n_origin=1008 * 5)
    with pytest.raises(_lib.Ft8rxError, match="m_lo"):
        dw.reference_stream(x, dw.IQ_I16, rate, 0.0, 10, 10)
    with pytest.raises(_lib.Ft8rxError, match="f_dial_hz"):
        dw.reference(x, dw.IQ_I16, rate, 0.5 * rate)
    with pytest.raises(_lib.Ft8rxError, match="15 s"):
        dw.reference(np.zeros(15 * rate + 1, np.int16), dw.REAL_I16, rate, 0.0)


# ---- end to end
@pytest.mark.parametrize("i", [0, 1, 2])
def test_two_channels_through_twin_and_oracle(i):
    """a_i and b_i in one 240 kHz IQ int16 stream, a strong tone next to each: the oracle decodes from the twin's frame what it decodes
    from the original frame"""
    iq, offs, originals = cases.recipe(i, 20)
    for j, (f_off, original) in enumerate(zip(offs, originals)):
        y, _ = dw.reference(iq, dw.IQ_I16, 240000, f_off)
        got, want = cases.oracle_texts(cases.to_frame(y)), cases.oracle_texts(original)
        print(f"i={i} channel {'ab'[j]}: {len(got)} messages, original frame {len(want)}")
        assert got == want and len(want) >= 5


# ---- the index arithmetic under the host sanitizers
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_ring_arithmetic_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ddc_wide_ring_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "ddc_wide_ring_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr
    assert "ddc wide ring arithmetic:" in p.stdout and int(p.stdout.split(":")[1].split()[0]) > 100000
    # the Python twin of the one-shot count is the header's (the program checks 719756 for 15 s less 1237 samples at 240 kHz)
    assert dw.mid_count(15 * 240000 - 1237, 240000) == 719756 and dw.mid_count(0, 240000) == 1 and dw.mid_count(15 * 240000, 240000) == 720000
