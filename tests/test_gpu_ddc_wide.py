"""The wide pre-decimator on the GPU (ft8rx_ddc_wide*): single taps against the float64 twin
(pyft8_amd/ddc_wide.py) by impulses, the whole chain against the twin on full-scale random input of every kind, chunk invariance across
the history wrap and across n = 2^32, the one-shot against the stream byte for byte, decode end to end (batch and live), the refusals
and the untouched default path.

Error of the float32 output against the twin, three channels (counts; measured on an MI355X, printed by test_twin_*; the bound is
derived, see bound()):
  one-shot 240 kHz, gain 0.75, real int16 / IQ int16 / IQ uint8 / IQ int8:  max 0.0090 / 0.0079 / 0.0072 / 0.0062, rms 0.00088 /
                                                                            0.00062 / 0.00062 / 0.00062 (bound 6.90 / 4.88 / 4.86 / 4.88)
  one-shot 384 kHz / 768 kHz IQ int16, gain 0.75:                           max 0.0048 / 0.0040, rms 0.00053 / 0.00037 (bound 5.09 / 5.44)
  stream 2.4 MHz IQ uint8, 4 tiles:                                         max 0.0023, rms 0.00029 (bound 8.77)
  stream 64.8 MHz real int16, 2 tiles:                                      max 0.00060, rms 0.000083 (bound 108.8)
  a single tap (test_impulse), relative to its value:                       1.2e-7 (bound 8 x 2^-23 = 9.5e-7)"""

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import ddc_cases as cases
from conftest import load_golden
from pyft8_amd import _lib, ddc
from pyft8_amd import ddc_wide as dw
from pyft8_amd.receiver import Receiver

pytestmark = pytest.mark.gpu

NSAMP = 180000
TILE = 1008
BANDS = ["40m", "60m"]


def dials(rate):
    """negative and within 1 kHz of -rate/2; positive; within 1 kHz of +rate/2 (dial + 3000 wraps)"""
    return [-0.5 * rate + 400.0, 0.11 * rate, 0.5 * rate - 700.0]


def g0(kind):
    return 1.0 if dw.is_iq(kind) else 2.0


def bound(kind, rate, gain, xmax):
    """The project's bound (tests/test_gpu_ddc.py) with the pre-stage in front: (n_macs + 24) 2^-23 G max|x|, n_macs = len(h0) + len(h1) +
    len(h2) multiply-adds on the path into one output, G = gain g0 sum|h0| sum|h1| sum|h2|.  Each float32 operation adds at most 2^-24
    of the magnitudes summed so far; the 24 covers the rounded tables of both stages, their products, the rotation, the mixing
    products and the scalings."""
    mid = dw.plan(rate)[0]
    h = [dw.taps(rate), ddc.taps(mid, 1), ddc.taps(mid, 2)]
    G = gain * g0(kind) * np.prod([np.abs(t.astype(np.float64)).sum() for t in h])
    return (sum(len(t) for t in h) + 24) * 2.0 ** -23 * G * xmax


_data = {}


def samples(kind, n, key):
    """Full-scale random samples of one stream of `kind`, the corners of the range at both ends"""
    if (kind, n, key) not in _data:
        rng = np.random.Generator(np.random.Philox(key=0x51DE + key))
        info = np.iinfo(dw._DTYPE[kind])
        x = rng.integers(info.min, info.max + 1, size=(n, 2) if dw.is_iq(kind) else n, dtype=np.int64).astype(dw._DTYPE[kind])
        x[:3], x[-3:] = info.max, info.min
        x.setflags(write=False)
        _data[(kind, n, key)] = x
    return _data[(kind, n, key)]


def xmax_of(x, kind):
    v = dw.sample_values(x, kind)
    return float(np.abs(v).max())


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle(device=0, max_frames=3)
    yield h
    h.close()


@pytest.fixture()
def stream(handle):
    """open(...) opens the handle's wide stream; it is closed after the test whatever happened"""
    def open_(kind, rate, f=None, **kw):
        return handle.ddc_wide_stream_open(kind, rate, dials(rate) if f is None else f, keep_f32=True, **kw)
    yield open_
    if handle._wds is not None:
        handle.ddc_wide_stream_close()


def push_all(handle, x, rate, **kw):
    m = None
    for at in range(0, len(x), rate):
        m = handle.ddc_wide_stream_push(x[at:at + rate], **kw)
    return m


# ---- single taps
def origin_below_2_32(rate):
    grid = TILE * rate // 12000
    n_origin = (2 ** 32 - 2 * grid - 1) // grid * grid
    assert n_origin % grid == 0 and n_origin < 2 ** 32 - 2 * grid <= n_origin + grid
    return n_origin


def impulse_positions(rate):
    """(name, n_origin, n) of the six impulses.  The stream is pushed in one piece, so the kernel's tiles begin at k_origin."""
    _, R0 = dw.plan(rate)
    C0 = (len(dw.taps(rate)) - 1) // 2
    tk = min(16, (6144 - 1024) // R0 + 1)                       # csrc/ddc_wide_ring.hpp: tile_outputs
    k0, k1 = 40 * tk, 41 * tk + 3
    near = origin_below_2_32(rate)
    return [("first input of a tile", 0, k0 * R0 - C0), ("last input of a tile", 0, (k0 + tk - 1) * R0 + C0),
            ("k R0 + C0", 0, k1 * R0 + C0), ("k R0 - C0", 0, k1 * R0 - C0), ("n = 2^32 - 1", near, 2 ** 32 - 1), ("n = 2^32", near, 2 ** 32)]


@pytest.mark.parametrize("rate,kind", [(240000, dw.IQ_I16), (2400000, dw.IQ_U8), (2400000, dw.IQ_I8)], ids=["240k-iq16", "2400k-u8", "2400k-i8"])
def test_impulse(handle, stream, rate, kind):
    """One full-scale sample (I = the most negative value, Q at rest) in a stream at rest: every intermediate sample it reaches is ONE
    product, tap j = n - (k R0 - C0), so a dropped, shifted or mis-phased tap shows.  Against reference_mid within
    8 x 2^-23 |h0[j]| 32768 g0 per sample (the table entry, its product with the sample, the rotation and their product: each at most
    2^-24 of |h0[j] x| per component) and exactly zero outside the filter's reach.
    IQ uint8 has no zero (x = 256 (u - 127.5)): there the stream rests at u = 128, x = 128 + 128i, and on top of the impulse's bound
    comes the background's by the same rule as bound(): (N0 + 8) 2^-23 sum|h0| 128 sqrt(2); outside the reach the twin's value is the
    background's response instead of zero.  The IQ int8 case at the same rate is the strict form of it."""
    _, R0 = dw.plan(rate)
    h0 = dw.taps(rate).astype(np.float64)
    N0, C0 = len(h0), (len(h0) - 1) // 2
    rest = 128 if kind == dw.IQ_U8 else 0
    low = np.iinfo(dw._DTYPE[kind]).min
    back = (N0 + 8) * 2.0 ** -23 * np.abs(h0).sum() * 128.0 * np.sqrt(2.0) if kind == dw.IQ_U8 else 0.0
    f = dials(rate)
    worst = 0.0
    for name, n_origin, n in impulse_positions(rate):
        x = np.full((n - n_origin + C0 + 60 * R0, 2), rest, dw._DTYPE[kind])
        x[n - n_origin, 0] = low
        assert len(x) <= rate and abs(dw.sample_values(x[n - n_origin:n - n_origin + 1], kind)[0].real) >= 32640
        stream(kind, rate, n_origin=n_origin)
        handle.ddc_wide_stream_push(x)
        k_origin = n_origin // R0
        k_lo, k_hi = max(k_origin, -(-(n - C0) // R0) - 40), (n + C0) // R0 + 41
        v = handle.ddc_wide_stream_read_mid(k_lo, k_hi - k_lo).astype(np.complex128)
        handle.ddc_wide_stream_close()
        j = n - (np.arange(k_lo, k_hi) * R0 - C0)
        inside = (j >= 0) & (j < N0)
        assert inside.sum() in (N0 // R0, N0 // R0 + 1) and not inside[:30].any() and not inside[-30:].any()
        lim = np.where(inside, 8 * 2.0 ** -23 * np.abs(h0[np.clip(j, 0, N0 - 1)]) * 32768.0, 0.0) + back
        for c in range(3):
            ref = dw.reference_mid(x, kind, rate, f[c], k_lo, k_hi, n_origin)
            err = np.abs(v[c] - ref)
            assert np.abs(v[c][inside]).max() > 300                                      # the impulse came through
            assert (err <= lim).all(), (name, c, int(np.argmax(err - lim)), float(err.max()))
            if kind != dw.IQ_U8:
                assert not v[c][~inside].any()
            worst = max(worst, float((err[inside] / (np.abs(ref[inside]) + 1e-30)).max()))
    print(f"ddc wide impulse rate {rate} {dw.KIND_NAMES[kind]}: worst relative error of a single tap {worst:.3e} (2^-23 = {2.0 ** -23:.3e})")


# ---- the whole chain against the twin
def against_twin(what, kind, rate, x, y, fm, m_lo, m_hi, n_origin=0, gain=1.0):
    lim = bound(kind, rate, gain, xmax_of(x, kind))
    worst = 0.0
    for c, f in enumerate(dials(rate)):
        ref = dw.reference_stream(x, kind, rate, f, m_lo, m_hi, n_origin=n_origin, gain=gain)
        err = y[c].astype(np.float64) - ref
        print(f"ddc wide twin {what}, channel {c}: max |err| {np.abs(err).max():.5f}, rms {np.sqrt((err ** 2).mean()):.6f} counts, "
              f"bound {lim:.4f}, rms of y {y[c].std():.1f}")
        assert ref.std() > 100 and 0.99 < y[c].std() / ref.std() < 1.01                 # a real signal came out
        assert abs(fm[c] - dw.frequency_words(rate, f)[3]) <= 1e-9 and abs(fm[c] - f) <= rate / 2.0 ** 32
        worst = max(worst, np.abs(err).max())
    assert worst <= lim


ONE_SHOT = [(k, 240000) for k in dw.KINDS] + [(dw.IQ_I16, 384000), (dw.IQ_I16, 768000)]


@pytest.mark.parametrize("kind,rate", ONE_SHOT, ids=[f"{dw.KIND_NAMES[k].replace(' ', '_')}-{r}" for k, r in ONE_SHOT])
def test_twin_one_shot(handle, kind, rate):
    """30000 outputs' worth of full-scale samples, less 1237: the first 30200 outputs against the twin, the zero tail, the frame"""
    D = rate // 12000
    n, m_hi = D * 30000 - 1237, 30200
    x = samples(kind, n, D)
    fm, y = handle.ddc_wide(x, kind, rate, dials(rate), gain=0.75, want_float=True)
    a = handle.download_audio(handle.staging_ptr(), 3)
    assert y.shape == (3, NSAMP) and np.isfinite(y).all()
    against_twin(f"one-shot {rate} {dw.KIND_NAMES[kind]}", kind, rate, x, y[:, :m_hi], fm, 0, m_hi, gain=0.75)
    assert np.array_equal(a, cases.to_frame(y))                                      # the frame is rint + saturation of the GPU's own y
    assert not y[:, 30000 + 300:].any() and not a[:, 30000 + 300:].any()              # beyond the input and the filters: the zero tail


@pytest.mark.parametrize("kind,rate,tiles", [(dw.IQ_U8, 2400000, 4), (dw.REAL_I16, 64800000, 2)], ids=["IQ_uint8-2400000", "real_int16-64800000"])
def test_twin_stream(handle, stream, kind, rate, tiles):
    D = rate // 12000
    n = (tiles * TILE + 160) * D                               # the tiles and the reach of the filters behind them (less than 150 outputs)
    x = samples(kind, n, D)
    fm = stream(kind, rate)
    m = push_all(handle, x, rate)
    assert m == tiles * TILE
    a, y = handle.ddc_stream_read(0, m, want_float=True)
    against_twin(f"stream {rate} {dw.KIND_NAMES[kind]}", kind, rate, x, y, fm, 0, m)
    assert np.array_equal(a, cases.to_frame(y))


def test_saturation(handle):
    """gain drives the output past full scale: -32768 / 32767, never a wrap"""
    rate, kind = 240000, dw.IQ_I8
    x = samples(kind, 20 * 6000, 3)
    fm, y = handle.ddc_wide(x, kind, rate, dials(rate), gain=24.0, want_float=True)
    a = handle.download_audio(handle.staging_ptr(), 3)
    assert y.max() > 2 * 32767 and y.min() < -2 * 32768 and np.array_equal(a, cases.to_frame(y))
    assert (a == 32767).sum() > 100 and (a == -32768).sum() > 100


# ---- invariance
def chunks_of(total, lens):
    out, i = [], 0
    while sum(out) < total:
        out.append(min(lens[i % len(lens)], total - sum(out)))
        i += 1
    return out


def test_chunk_invariance(handle, stream):
    """240 kHz from just below n = 2^32, pushed in 1-s chunks and in chunks cycling through 1, 479, 480 x 20, 7 x 20 + 3 and 3 (shorter
    than R0 = 5; the history of 37 samples wraps all the time), with a one-shot ft8rx_ddc at 48 kHz on the same handle in the middle:
    every output is the same bytes; so are a second run, the device form of the push, and a channel opened alone"""
    rate, D = 240000, 20
    n_origin = origin_below_2_32(rate)
    total = rate + rate // 2 + 77
    x = samples(dw.IQ_I16, total, 100)
    other = np.random.Generator(np.random.Philox(key=5)).integers(-3000, 3000, size=(1, 20000, 2)).astype(np.int16)
    m0 = n_origin // D
    got = []
    for run, lens in enumerate(([rate], [1, 479, 480 * D, 7 * D + 3, 3], [rate], [50001, 99999], [rate])):
        alone = run == 4
        fm = stream(dw.IQ_I16, rate, f=dials(rate)[1:2] if alone else None, n_origin=n_origin)
        at, m = 0, m0
        for n in chunks_of(total, lens):
            m_new = handle.ddc_wide_stream_push(x[at:at + n], device=(run == 3))
            assert m_new >= m and m_new % TILE == 0
            at, m = at + n, m_new
            if at >= total // 2 > at - n and run == 1:                                  # the plain one-shot uses nothing of the stream
                handle.ddc(other, ddc.IQ_I16, 48000, [0], [1000.0])
        info = handle.ddc_stream_info()
        assert info["m_produced"] == m and (m0 + 4 * TILE) * D > 2 ** 32 > n_origin
        assert m - m0 >= (total // D) - 2 * TILE - 100                                  # at most a tile and the filters' reach behind
        a, y = handle.ddc_stream_read(m0, m - m0, want_float=True)
        got.append((a[0:1], y[0:1], fm) if alone else (a, y, fm))
        handle.ddc_wide_stream_close()
    assert np.abs(got[0][1]).max() > 1000
    for other_run in got[1:4]:
        assert other_run[0].tobytes() == got[0][0].tobytes() and other_run[1].tobytes() == got[0][1].tobytes() and np.array_equal(other_run[2], got[0][2])
    assert got[4][0].tobytes() == got[0][0][1:2].tobytes() and got[4][1].tobytes() == got[0][1][1:2].tobytes() and got[4][2][0] == got[0][2][1]


def test_a_push_that_completes_nothing_makes_nothing(handle, stream):
    rate = 240000
    x = samples(dw.IQ_I16, 40000, 8)
    stream(dw.IQ_I16, rate)
    assert handle.ddc_wide_stream_push(x[:3]) == 0 and handle.ddc_wide_stream_push(x[3:16]) == 0          # v[0] needs input 16
    assert handle.ddc_stream_info()["n_pushed"] == 0
    assert handle.ddc_wide_stream_push(x[16:17]) == 0 and handle.ddc_stream_info()["n_pushed"] == 1
    assert handle.ddc_wide_stream_push(x[17:21]) == 0 and handle.ddc_stream_info()["n_pushed"] == 1        # v[1] needs input 21
    assert handle.ddc_wide_stream_push(x[21:]) == TILE and handle.ddc_stream_info()["n_pushed"] == (40000 - 17) // 5 + 1


@pytest.mark.parametrize("kind,rate", [(dw.IQ_I16, 240000), (dw.REAL_I16, 240000), (dw.IQ_U8, 2400000)], ids=["iq16-240k", "real-240k", "u8-2400k"])
def test_first_cycle_is_the_one_shot(handle, stream, kind, rate):
    """5000 outputs' worth of samples pushed, the same samples through ft8rx_ddc_wide (device and host entry): the four complete tiles
    are the same bytes, int16 and float32"""
    D = rate // 12000
    x = samples(kind, 5000 * D, 200 + D)
    fm1, y1 = handle.ddc_wide(x, kind, rate, dials(rate), want_float=True)
    a1 = handle.download_audio(handle.staging_ptr(), 3)
    fmh = handle.ddc_wide(x, kind, rate, dials(rate))                                  # the host entry
    assert np.array_equal(fmh, fm1) and handle.download_audio(handle.staging_ptr(), 3).tobytes() == a1.tobytes()
    # a channel computed alone is the same bytes
    fm_1, y_1 = handle.ddc_wide(x, kind, rate, dials(rate)[2:], want_float=True)
    assert y_1[0].tobytes() == y1[2].tobytes() and fm_1[0] == fm1[2]
    fm = stream(kind, rate)
    assert push_all(handle, x, rate) == 4 * TILE
    a, y = handle.ddc_stream_read(0, 4 * TILE, want_float=True)
    assert np.array_equal(fm, fm1) and np.abs(y).max() > 1000
    assert y.tobytes() == y1[:, :4 * TILE].tobytes() and a.tobytes() == a1[:, :4 * TILE].tobytes()


# ---- decode
@pytest.fixture(scope="module")
def rx():
    r = Receiver("", None, max_frames=2)
    yield r
    r.close()


def texts(dicts):
    return [" ".join(d["msg_tuple"]) for d in dicts]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_decode_stream(rx, i):
    """Two FT8 channels in one 240 kHz IQ int16 stream: every channel decodes to the message set of its original 12 kHz frame"""
    iq, offs, originals = cases.recipe(i, 20)
    want = rx.decode_frames(np.stack(originals))
    got = rx.decode_stream(iq, 240000, iq=True, dial_offsets_hz=offs, bands=BANDS)
    assert len(got) == 2
    for j in range(2):
        print(f"ddc wide decode i={i} channel {j}: {len(got[j])} messages, original frame {len(want[j])}")
        assert set(texts(got[j])) == set(texts(want[j])) and len(want[j]) >= 5
        assert all(d["band"] == BANDS[j] and 0.0 < d["fHz"] < 3000.0 for d in got[j])


def test_decode_stream_uint8_and_passes(rx):
    """The same stream as uint8 pairs, scaled so that the sum uses the 8-bit range: decoded, and compared with decode_frames on the
    twin's frames for that input.  passes=2 works on the frames the wide path left in the staging buffer: they are ordinary frames."""
    iq, offs, _ = cases.recipe(0, 20)
    scale = 127.0 / np.abs(iq.astype(np.int32)).max()
    u8 = np.clip(np.floor(iq.astype(np.float64) * scale + 128.0), 0, 255).astype(np.uint8)
    assert u8.min() <= 1 and u8.max() >= 254
    frames = np.stack([cases.to_frame(dw.reference(u8, dw.IQ_U8, 240000, f)[0]) for f in offs])
    want = rx.decode_frames(frames)
    got = rx.decode_stream(u8, 240000, iq=True, dial_offsets_hz=offs, bands=BANDS)
    for j in range(2):
        print(f"ddc wide decode uint8 channel {j}: {len(got[j])} messages, the twin's frame {len(want[j])}")
        assert set(texts(got[j])) == set(texts(want[j])) and len(want[j]) >= 3
    one = rx.decode_stream(iq, 240000, iq=True, dial_offsets_hz=offs)
    h = rx._handle(2)
    h.ddc_wide(iq, dw.IQ_I16, 240000, offs)
    frames = h.download_audio(h.staging_ptr(), 2)
    two = rx.decode_stream(iq, 240000, iq=True, dial_offsets_hz=offs, passes=2)
    want = rx.decode_frames(frames, passes=2)
    for j in range(2):
        assert texts(two[j])[:len(one[j])] == texts(one[j])                           # the first pass, then what subtraction adds
        assert texts(two[j]) == texts(want[j]) and [d["decode_notes"] for d in two[j]] == [d["decode_notes"] for d in want[j]]
    # what the wide path does not take
    for bad, kw, word in ((iq.astype(np.float32), {"iq": True}, "float32"), (iq[:, 0] + 1j * iq[:, 1], {"iq": True}, "complex"),
                          (np.stack([iq, iq]), {"iq": True}, "one stream"), (iq[:, 0].astype(np.float64), {}, "float64")):
        with pytest.raises(_lib.Ft8rxError, match=word):
            rx.decode_stream(bad, 240000, dial_offsets_hz=offs, **kw)
    with pytest.raises(_lib.Ft8rxError, match="rate"):
        rx.decode_stream(iq, 250000, iq=True, dial_offsets_hz=offs)


def live_chunks(x):
    """The stream in chunks of 38400 and 20000 samples alternately -> (chunk, samples pushed once it is in)"""
    at, i = 0, 0
    while at < len(x):
        n = (38400, 20000)[i % 2]
        yield x[at:at + n], min(at + n, len(x))
        at, i = at + n, i + 1


def test_live_end_to_end(rx):
    """One cycle of 240 kHz IQ int16 with two channels through Receiver(sample_rate=...), pushed in uneven chunks with a poll() after
    each: every message of decode_stream arrives once per channel, with its channel and band, some of them early, before the cycle's
    last sample has been pushed"""
    import time as _t
    iq, offs, _ = cases.recipe(0, 20)
    rate, t_first = 240000, 15.0 * 1000
    want = [set(texts(lst)) for lst in rx.decode_stream(iq, rate, iq=True, dial_offsets_hz=offs)]
    cs = _t.strftime("%y%m%d_%H%M%S", _t.gmtime(t_first))
    vt, pushed, got = [t_first], [0], []
    live = Receiver("x", lambda d: got.append((pushed[0], d)), time_source=lambda: vt[0], sample_rate=rate, iq=True, dial_offsets_hz=offs,
                    bands=BANDS, t_first=t_first)
    try:
        assert live._thread is None and live.wide_in.n_channels == 2 and live.wide_in.wide
        returned = []
        for chunk, n in live_chunks(iq):
            pushed[0], vt[0] = n, t_first + n / rate
            live.wide_in.push(chunk)
            returned += live.poll()
        live.wide_in.flush()
        returned += live.poll()
        assert live._live.max_frames == 2 and live.wide_in.n_pushed == len(iq)
    finally:
        live.stop()
    assert returned == [d for _, d in got]
    for j in range(2):
        lst = [(n, d) for n, d in got if d["channel"] == j]
        assert all(d["band"] == BANDS[j] and d["cyclestart_string"] == cs and 0.0 < d["fHz"] < 3000.0 for _, d in lst)
        t = texts([d for _, d in lst])
        print(f"live wide channel {j}: {len(t)} messages, {sum(d['early'] for _, d in lst)} early")
        assert len(set(t)) == len(t) and set(t) == want[j] and len(t) >= 5
        assert all(n < len(iq) for n, d in lst if d["early"]) and all(n >= len(iq) for n, d in lst if not d["early"])
    assert any(d["early"] for _, d in got)


# ---- refusals
def test_refusals_and_untouched_default_path(handle):
    audio = np.stack([load_golden(n)[0] for n in ("test_08", "synth_000000")])
    before = handle.decode_batch(audio)
    L, h = handle._L, handle._h
    rate = 240000
    x = np.zeros((rate + 1, 2), np.int16)
    f, fm = np.array(dials(rate) + [0.0]), np.zeros(4)

    def err():
        return L.ft8rx_last_error(h).decode()

    def call(kind=dw.IQ_I16, rate=rate, n=1000, n_out=3):
        return L.ft8rx_ddc_wide_host(h, x.ctypes.data, kind, rate, n, n_out, f.ctypes.data, 1.0, fm.ctypes.data)

    def open_(kind=dw.IQ_I16, rate=rate, n_out=3, n_origin=0):
        return L.ft8rx_ddc_wide_stream_open(h, kind, rate, n_out, f.ctypes.data, 1.0, n_origin, 0, None)

    assert call() == 0
    # nothing is open yet
    assert L.ft8rx_ddc_wide_stream_push(h, x.ctypes.data, 1000, 0, None) == -1 and "no wide stream is open" in err()
    assert L.ft8rx_ddc_wide_stream_read_mid(h, 0, 10, fm.ctypes.data) == -1 and "no wide stream is open" in err()
    assert L.ft8rx_ddc_wide_stream_close(h) == -1
    with pytest.raises(_lib.Ft8rxError, match="no wide stream is open"):
        handle.ddc_wide_stream_push(x[:100])
    for fn in (call, open_):
        for kw, word in (({"kind": ddc.IQ_I16}, "kind"), ({"kind": 20}, "kind"), ({"kind": 15}, "kind"), ({"rate": 250000}, "rate_hz"),
                         ({"rate": 2048000}, "rate_hz"), ({"rate": 192000}, "rate_hz"), ({"rate": 144000}, "rate_hz"), ({"rate": 129648000}, "rate_hz"),
                         ({"n_out": 4}, "n_out"), ({"n_out": 0}, "n_out")):
            assert fn(**kw) == -1 and word in err(), (fn.__name__, kw, err())
        f[1] = 0.5 * rate
        assert fn() == -1 and "f_dial_hz[1]" in err()
        f[1] = -0.5 * rate - 1.0
        assert fn() == -1 and "f_dial_hz[1]" in err()
        f[1] = dials(rate)[1]
    assert call(n=15 * rate + 1) == -1 and "n_samples" in err()
    assert L.ft8rx_ddc_wide(h, None, dw.IQ_I16, rate, 1000, 3, f.ctypes.data, 1.0, None, None, None) == -1 and "d_in" in err()
    for n_origin in (1008, 1008 * 20 + 5, 1008 * 5, 1008 * 4):
        assert open_(n_origin=n_origin) == -1 and "n_origin" in err()
    assert open_(rate=768000, n_origin=1008 * 20) == -1 and "n_origin" in err()
    with pytest.raises(_lib.Ft8rxError, match="kind"):
        handle.ddc_wide(x[:100], 7, rate, [0.0])
    # one wide stream per handle; while it is open the plain stream and the wide one-shot are refused
    assert open_(n_origin=1008 * 20 * 3) == 0
    assert open_() == -1 and "open on this handle already" in err()
    src = np.zeros(3, np.int32)
    assert L.ft8rx_ddc_stream_open(h, ddc.IQ_I16, 48000, 1, 3, src.ctypes.data, f.ctypes.data, 1.0, 0, 0, None) == -1 and "wide stream is open" in err()
    assert L.ft8rx_ddc_stream_push(h, x.ctypes.data, 100, 0, None) == -1 and "wide stream" in err()
    assert L.ft8rx_ddc_stream_close(h) == -1 and "wide stream" in err()
    assert call() == -1 and "wide stream is open" in err()
    for n_new in (0, rate + 1):
        assert L.ft8rx_ddc_wide_stream_push(h, x.ctypes.data, n_new, 0, None) == -1 and "n_new" in err()
    assert L.ft8rx_ddc_wide_stream_push(h, None, 100, 0, None) == -1 and "in is NULL" in err()
    m = np.zeros(1, np.uint64)
    assert L.ft8rx_ddc_wide_stream_push(h, x.ctypes.data, rate, 0, m.ctypes.data) == 0 and 1008 * 3 < int(m[0]) <= 1008 * 3 + 12000
    assert L.ft8rx_ddc_wide_stream_read_mid(h, 0, 10, fm.ctypes.data) == -1 and "not all held" in err()
    mid = handle.decode_batch(audio)                                                 # a decode while the stream is open
    assert L.ft8rx_ddc_wide_stream_close(h) == 0
    assert L.ft8rx_ddc_wide_stream_push(h, x.ctypes.data, 1000, 0, None) == -1 and "no wide stream is open" in err()
    assert open_() == 0 and L.ft8rx_ddc_wide_stream_close(h) == 0                    # close, then open again
    f48 = np.zeros(3)
    assert L.ft8rx_ddc_stream_open(h, ddc.IQ_I16, 48000, 1, 3, src.ctypes.data, f48.ctypes.data, 1.0, 0, 0, None) == 0
    assert open_() == -1 and "a stream is open on this handle already" in err()      # ... and not beside a plain stream
    assert L.ft8rx_ddc_stream_close(h) == 0
    assert call() == 0                                                               # and a good call still runs
    after = handle.decode_batch(audio)
    for other in (mid, after):
        assert before[1].tobytes() == other[1].tobytes() and before[3].tobytes() == other[3].tobytes() and before[1].min() > 0
        for fr in range(2):
            nc, ne = int(before[1][fr]), min(int(before[3][fr]), _lib.EVENT_CAP)
            assert before[0][fr, :nc].tobytes() == other[0][fr, :nc].tobytes()
            assert sorted(e.tobytes() for e in before[2][fr, :ne]) == sorted(e.tobytes() for e in other[2][fr, :ne])
