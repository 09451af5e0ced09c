"""The rational resampler on the GPU (ft8rx_ddc_rat*): the whole chain against the float64 twin
(pyft8_amd/ddc_rat.py) on full-scale random input in both kernel regimes, single taps against the twin by impulses, the stream against
the one-shot byte for byte, chunk invariance across n = 2^32, decode end to end (batch and live), the refusals and the untouched
default paths.

Error of the float32 output against the twin, three channels, gain 0.75, 0.1 s of input (counts; measured on an MI355X, printed by
test_twin_one_shot; the bound is derived, see bound()):
  44100 real int16 (P = 7) / 22050 real float32 (P = 8, L = 320):  max 0.0124 / 0.0238, rms 0.0019 / 0.0025 (bound 6.94 / 7.59)
  250 kHz IQ uint8 (P = 33) / 2.048 MHz IQ int8 (P = 60):          max 0.0042 / 0.0016, rms 0.00060 / 0.00024 (bound 4.85 / 5.85)
  1 MS/s IQ int16 (P = 130) / 10 MS/s IQ int8 (P = 1291):          max 0.0028 / 0.0010, rms 0.00028 / 0.000095 (bound 6.19 / 22.0)
  a single tap (test_impulse), relative to its value:              1.0e-7 at 44100, 1.1e-7 at 10 MS/s (bound 8 x 2^-23 = 9.5e-7)"""
import threading
import time as _t

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import ddc_cases as cases
import ddc_rat_cases as rcases
from conftest import load_golden
from pyft8_amd import _lib, ddc
from pyft8_amd import ddc_rat as dr
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
    return 1.0 if dr.is_iq(kind) else 2.0


def geometry(rate):
    """(L, M, N, C, P, tk): the plan and the kernel's tile (csrc/ddc_rat_ring.hpp: lane_regime, tile_outputs)"""
    _, L, M, N = dr.plan(rate)
    P = -(-N // L)
    lane = P <= 64 and P * L <= 3072
    tk = min(256, (3200 - P - 1) * L // M + 1) if lane else min(16, (6144 - 1024 - 1) * L // M + 1)
    return L, M, N, (N - 1) // 2, P, tk


def phase_sum(rate):
    """max over the phases of sum_i |h[phi + i L]|: the gain of the resampler for the worst input"""
    return float(np.abs(dr.phase_table(rate)).sum(axis=1).max())


def bound(kind, rate, gain, xmax):
    """The project's bound (tests/test_gpu_ddc.py) with the resampler in front: (n_macs + 24) 2^-23 G max|x|, n_macs = P + len(h1) +
    len(h2) multiply-adds on the path into one output, G = gain g0 max_phi sum_i |h[phi + i L]| sum|h1| sum|h2|.  Each float32 operation
    adds at most 2^-24 of the magnitudes summed so far; the 24 covers the rounded tables of both stages, their products, the rotation,
    the mixing products and the scalings."""
    mid = dr.plan(rate)[0]
    h1, h2 = ddc.taps(mid, 1), ddc.taps(mid, 2)
    G = gain * g0(kind) * phase_sum(rate) * np.abs(h1.astype(np.float64)).sum() * np.abs(h2.astype(np.float64)).sum()
    return (geometry(rate)[4] + len(h1) + len(h2) + 24) * 2.0 ** -23 * G * xmax


_data = {}


def samples(kind, n, key):
    """Full-scale random samples of one stream of `kind`, the corners of the range at both ends"""
    if (kind, n, key) not in _data:
        rng = np.random.Generator(np.random.Philox(key=0x7A7 + key))
        shape = (n, 2) if dr.is_iq(kind) else n
        if kind in (dr.REAL_F32, dr.IQ_F32):
            x = rng.uniform(-32768.0, 32767.0, size=shape).astype(np.float32)
            lo, hi = -32768.0, 32767.0
        else:
            info = np.iinfo(dr._DTYPE[kind])
            x = rng.integers(info.min, info.max + 1, size=shape, dtype=np.int64).astype(dr._DTYPE[kind])
            lo, hi = info.min, info.max
        x[:3], x[-3:] = hi, lo
        x.setflags(write=False)
        _data[(kind, n, key)] = x
    return _data[(kind, n, key)]


def xmax_of(x, kind):
    return float(np.abs(dr.sample_values(x, kind)).max())


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle(device=0, max_frames=3)
    yield h
    h.close()


@pytest.fixture()
def stream(handle):
    """open(...) opens the handle's rational stream; it is closed after the test whatever happened"""
    def open_(kind, rate, f=None, **kw):
        return handle.ddc_rat_stream_open(kind, rate, dials(rate) if f is None else f, keep_f32=True, **kw)
    yield open_
    if handle._rts is not None:
        handle.ddc_rat_stream_close()


def push_all(handle, x, rate, **kw):
    m = None
    for at in range(0, len(x), rate):
        m = handle.ddc_rat_stream_push(x[at:at + rate], **kw)
    return m


def origin_grid(rate):
    """The smallest valid origin above 0: a whole number of tiles of the stage behind whose input time is an integer"""
    mid, L, M, _ = dr.plan(rate)
    gk = TILE * (mid // 12000)
    step = gk
    while (step * M) % L:
        step += gk
    return step * M // L


def origin_below_2_32(rate, room):
    """The last valid origin that leaves `room` inputs before n = 2^32"""
    grid = origin_grid(rate)
    n_origin = (2 ** 32 - room) // grid * grid
    assert dr.origin_ok(n_origin, rate) and n_origin + room <= 2 ** 32 < n_origin + room + grid
    return n_origin


# ---- the whole chain against the twin
ONE_SHOT = [(44100, dr.REAL_I16), (22050, dr.REAL_F32), (250000, dr.IQ_U8), (2048000, dr.IQ_I8), (1000000, dr.IQ_I16), (10000000, dr.IQ_I8)]


@pytest.mark.parametrize("rate,kind", ONE_SHOT, ids=[f"{r}-{dr.KIND_NAMES[k].replace(' ', '_')}" for r, k in ONE_SHOT])
def test_twin_one_shot(handle, rate, kind):
    """0.1 s of full-scale samples: the outputs they reach against the twin, the zero tail, the frame.  Lane regime: P = 7 (44100), 8
    (22050, the largest L), 33 (250 kHz), 60 (2.048 MHz); wave regime: P = 130 (1 MS/s), 1291 (10 MS/s)"""
    n, m_hi, gain = rate // 10, 1500, 0.75
    x = samples(kind, n, rate // 1000)
    fm, y = handle.ddc_rat(x, kind, rate, dials(rate), gain=gain, want_float=True)
    a = handle.download_audio(handle.staging_ptr(), 3)
    assert y.shape == (3, NSAMP) and np.isfinite(y).all()
    lim = bound(kind, rate, gain, xmax_of(x, kind))
    worst = 0.0
    for c, f in enumerate(dials(rate)):
        ref = dr.reference_stream(x, kind, rate, f, 0, m_hi, gain=gain)
        err = y[c, :m_hi].astype(np.float64) - ref
        print(f"ddc rat twin one-shot {rate} {dr.KIND_NAMES[kind]} (P = {geometry(rate)[4]}), channel {c}: max |err| {np.abs(err).max():.5f}, "
              f"rms {np.sqrt((err ** 2).mean()):.6f} counts, bound {lim:.4f}, rms of y {y[c, :1200].std():.1f}")
        assert ref[:1200].std() > 100 and 0.99 < y[c, :1200].std() / ref[:1200].std() < 1.01       # a real signal came out
        assert abs(fm[c] - dr.frequency_words(rate, f)[3]) <= 1e-9 and abs(fm[c] - f) <= rate / 2.0 ** 32
        worst = max(worst, np.abs(err).max())
    assert worst <= lim
    assert np.array_equal(a, cases.to_frame(y))                                      # the frame is rint + saturation of the GPU's own y
    assert not y[:, 1200 + 300:].any() and not a[:, 1200 + 300:].any()                # beyond the input and the filters: the zero tail


# ---- single taps
def impulse_positions(rate):
    """(name, n_origin, n) of the six impulses.  The stream is pushed in one piece, so the kernel's tiles begin at k_origin."""
    L, M, N, C, P, tk = geometry(rate)
    k0 = 40 * tk
    b = lambda k: (k * M + C) // L                                                   # noqa: E731 -- the last input of k
    k_a = next(k for k in range(41 * tk + 3, 41 * tk + 3 + L) if (k * M + C) % L == 0)
    k_b = next(k for k in range(43 * tk + 1, 43 * tk + 1 + L) if (k * M + C) % L == L - 1)
    near = origin_below_2_32(rate, 100 * M // L + 2 * P + 200)                       # the window of 40 outputs before the impulse lies behind the origin
    return [("first input of a tile", 0, b(k0) - P + 1), ("last input of a tile", 0, b(k0 + tk - 1)), ("phase 0", 0, b(k_a)),
            ("phase L - 1", 0, b(k_b)), ("n = 2^32 - 1", near, 2 ** 32 - 1), ("n = 2^32", near, 2 ** 32)]


@pytest.mark.parametrize("rate,kind", [(44100, dr.REAL_I16), (10000000, dr.IQ_I8), (2048000, dr.IQ_U8)], ids=["44100-real16", "10M-i8", "2048k-u8"])
def test_impulse(handle, stream, rate, kind):
    """One full-scale sample (the most negative value; Q at rest) in a stream at rest: every intermediate sample k it reaches is ONE
    product, tap j = t_k - n L, so a dropped, shifted or mis-phased tap shows.  Against reference_mid within
    8 x 2^-23 |h[j]| 32768 g0 per sample (the table entry, its product with the sample, the rotation and their product: each at most
    2^-24 of |h[j] x| per component) and exactly zero outside the filter's reach.
    IQ uint8 has no zero (x = 256 (u - 127.5)): there the stream rests at u = 128, x = 128 + 128i, and on top of the impulse's bound
    comes the background's by the same rule as bound(): (P + 8) 2^-23 max_phi sum_i |h[phi + i L]| 128 sqrt(2); outside the reach the
    twin's value is the background's response instead of zero."""
    L, M, N, C, P, _ = geometry(rate)
    h = dr.taps(rate).astype(np.float64)
    rest = 128 if kind == dr.IQ_U8 else 0
    low = np.iinfo(dr._DTYPE[kind]).min
    back = (P + 8) * 2.0 ** -23 * phase_sum(rate) * 128.0 * np.sqrt(2.0) if kind == dr.IQ_U8 else 0.0
    f = dials(rate)
    worst = 0.0
    for name, n_origin, n in impulse_positions(rate):
        x = np.full((n - n_origin + (2 * C + 60 * M) // L + 2,) + ((2,) if dr.is_iq(kind) else ()), rest, dr._DTYPE[kind])
        x[(n - n_origin, 0) if dr.is_iq(kind) else n - n_origin] = low
        assert len(x) <= rate and abs(dr.sample_values(x[n - n_origin:n - n_origin + 1], kind)[0].real) >= 32640
        stream(kind, rate, n_origin=n_origin)
        handle.ddc_rat_stream_push(x)
        k_origin = n_origin * L // M
        k_lo, k_hi = max(k_origin, -(-(n * L - C) // M) - 40), (n * L + C) // M + 41
        v = handle.ddc_rat_stream_read_mid(k_lo, k_hi - k_lo).astype(np.complex128)
        handle.ddc_rat_stream_close()
        j = np.arange(k_lo, k_hi) * M + C - n * L
        inside = (j >= 0) & (j < N)
        assert inside.sum() in (N // M, N // M + 1) and not inside[:30].any() and not inside[-30:].any()
        lim = np.where(inside, 8 * 2.0 ** -23 * np.abs(h[np.clip(j, 0, N - 1)]) * 32768.0 * g0(kind), 0.0) + back
        for c in range(3):
            ref = dr.reference_mid(x, kind, rate, f[c], k_lo, k_hi, n_origin)
            err = np.abs(v[c] - ref)
            assert np.abs(v[c][inside]).max() > 0.4 * 32640 * g0(kind) * h.max()            # the impulse came through: a tap of the main lobe
            assert (err <= lim).all(), (name, c, int(np.argmax(err - lim)), float(err.max()))
            if kind != dr.IQ_U8:
                assert not v[c][~inside].any()
            big = inside & (np.abs(ref) > 1e-3)
            worst = max(worst, float((err[big] / np.abs(ref[big])).max()))
    print(f"ddc rat impulse rate {rate} {dr.KIND_NAMES[kind]}: worst relative error of a single tap {worst:.3e} (2^-23 = {2.0 ** -23:.3e})")


# ---- invariance
def test_first_tiles_of_a_stream_are_the_one_shot(handle, stream):
    """44100 Hz real int16, 5000 outputs' worth of samples pushed, the same samples through ft8rx_ddc_rat (device and host entry): the
    first two tiles (2016 outputs) are the same bytes, int16 and float32; so is a channel computed alone"""
    rate, kind = 44100, dr.REAL_I16
    x = samples(kind, 5000 * rate // 12000, 200)
    fm1, y1 = handle.ddc_rat(x, kind, rate, dials(rate), want_float=True)
    a1 = handle.download_audio(handle.staging_ptr(), 3)
    fmh = handle.ddc_rat(x, kind, rate, dials(rate))                                   # the host entry
    assert np.array_equal(fmh, fm1) and handle.download_audio(handle.staging_ptr(), 3).tobytes() == a1.tobytes()
    fm_1, y_1 = handle.ddc_rat(x, kind, rate, dials(rate)[2:], want_float=True)
    assert y_1[0].tobytes() == y1[2].tobytes() and fm_1[0] == fm1[2]
    fm = stream(kind, rate)
    m = push_all(handle, x, rate)
    assert m >= 2 * TILE and m % TILE == 0
    a, y = handle.ddc_stream_read(0, 2 * TILE, want_float=True)
    assert np.array_equal(fm, fm1) and np.abs(y).max() > 1000
    assert y.tobytes() == y1[:, :2 * TILE].tobytes() and a.tobytes() == a1[:, :2 * TILE].tobytes()


def chunks_of(total, lens):
    out, i, done = [], 0, 0
    while done < total:
        out.append(min(lens[i % len(lens)], total - done))
        done += out[-1]
        i += 1
    return out


@pytest.mark.parametrize("rate", [2048000, 10000000], ids=["2048k", "10M"])
def test_chunk_invariance(handle, stream, rate):
    """IQ int8 from a valid origin just below n = 2^32, pushed in 1-s chunks and in chunks cycling through 1, M - 1, 9600, a prime and 3
    (the history of P samples wraps all the time), with a one-shot ft8rx_ddc at 48 kHz on the same handle in the middle: every output is
    the same bytes; so are the device form of the push and a channel opened alone"""
    kind = dr.IQ_I8
    mid, L, M, _ = dr.plan(rate)
    n_origin = origin_below_2_32(rate, 1000)
    total = 2 ** 32 - n_origin + rate // 5                                           # across n = 2^32 and 0.2 s beyond
    assert total <= 2 * rate
    x = samples(kind, total, 100)
    other = np.random.Generator(np.random.Philox(key=5)).integers(-3000, 3000, size=(1, 20000, 2)).astype(np.int16)
    m0 = n_origin * 12000 // rate
    assert m0 * rate == n_origin * 12000 and m0 % TILE == 0
    got = []
    for run, lens in enumerate(([rate], [1, M - 1, 9600, 7919, 3], [50001, 99999], [1, M - 1, 9600, 7919, 3])):
        alone = run == 3
        fm = stream(kind, rate, f=dials(rate)[1:2] if alone else None, n_origin=n_origin)
        at, m = 0, m0
        for n in chunks_of(total, lens):
            m_new = handle.ddc_rat_stream_push(x[at:at + n], device=(run == 2))
            assert m_new >= m and m_new % TILE == 0
            at, m = at + n, m_new
            if at >= total // 2 > at - n and run == 1:                                  # the plain one-shot is not refused and uses nothing of the stream
                handle.ddc(other, ddc.IQ_I16, 48000, [0], [1000.0])
        info = handle.ddc_stream_info()
        assert info["m_produced"] == m and m > m0 + TILE
        assert m - m0 >= total * 12000 // rate - 2 * TILE - 100                         # at most a tile and the filters' reach behind
        a, y = handle.ddc_stream_read(m0, m - m0, want_float=True)
        got.append((a[0:1], y[0:1], fm) if alone else (a, y, fm))
        handle.ddc_rat_stream_close()
    assert np.abs(got[0][1]).max() > 1000
    for other_run in got[1:3]:
        assert other_run[0].tobytes() == got[0][0].tobytes() and other_run[1].tobytes() == got[0][1].tobytes() and np.array_equal(other_run[2], got[0][2])
    assert got[3][0].tobytes() == got[0][0][1:2].tobytes() and got[3][1].tobytes() == got[0][1][1:2].tobytes() and got[3][2][0] == got[0][2][1]


def test_a_push_that_completes_nothing_makes_nothing(handle, stream):
    """44100 Hz: v[0] needs input (C) / L = 503 / 160 = 3, v[1] input (147 + 503) / 160 = 4"""
    rate = 44100
    x = samples(dr.REAL_I16, 10000, 8)
    stream(dr.REAL_I16, rate)
    assert handle.ddc_rat_stream_push(x[:3]) == 0 and handle.ddc_stream_info()["n_pushed"] == 0
    assert handle.ddc_rat_stream_push(x[3:4]) == 0 and handle.ddc_stream_info()["n_pushed"] == 1
    assert handle.ddc_rat_stream_push(x[4:5]) == 0 and handle.ddc_stream_info()["n_pushed"] == 3            # v[1] and v[2]: inputs 4 and 4
    assert handle.ddc_rat_stream_push(x[5:]) == 2 * TILE
    assert handle.ddc_stream_info()["n_pushed"] == (10000 * 160 - 503 - 1) // 147 + 1


# ---- decode
@pytest.fixture(scope="module")
def rx():
    r = Receiver("", None, max_frames=2)
    yield r
    r.close()


def texts(dicts):
    return [" ".join(d["msg_tuple"]) for d in dicts]


def test_decode_stream(rx):
    """Two FT8 channels in one 250 kHz IQ int16 stream: every channel decodes to the message set of its original 12 kHz frame; without
    resample=True the rate is refused as it always was"""
    iq, offs, originals = rcases.recipe(0, 250000, True)
    want = rx.decode_frames(np.stack(originals))
    got = rx.decode_stream(iq, 250000, iq=True, dial_offsets_hz=offs, bands=BANDS, resample=True)
    assert len(got) == 2
    for j in range(2):
        print(f"ddc rat decode channel {j}: {len(got[j])} messages, original frame {len(want[j])}")
        assert set(texts(got[j])) == set(texts(want[j])) and len(want[j]) >= 5
        assert all(d["band"] == BANDS[j] and 0.0 < d["fHz"] < 3000.0 for d in got[j])
    with pytest.raises(_lib.Ft8rxError, match="rate"):
        rx.decode_stream(iq, 250000, iq=True, dial_offsets_hz=offs)
    with pytest.raises(_lib.Ft8rxError, match="rate"):
        rx.decode_stream(iq[:, 0].copy(), 44100)
    with pytest.raises(_lib.Ft8rxError, match="900001"):
        rx.decode_stream(iq, 900001, iq=True, dial_offsets_hz=offs, resample=True)
    with pytest.raises(_lib.Ft8rxError, match="one stream"):
        rx.decode_stream(np.stack([iq, iq]), 250000, iq=True, dial_offsets_hz=offs, resample=True)
    # with the flag, the rates of the other two paths take those paths: the same bytes as without it
    iq48, offs48, _ = cases.recipe(0, 4)
    assert [texts(c) for c in rx.decode_stream(iq48, 48000, iq=True, dial_offsets_hz=offs48, resample=True)] == \
           [texts(c) for c in rx.decode_stream(iq48, 48000, iq=True, dial_offsets_hz=offs48)]


def test_live_end_to_end(rx):
    """One cycle of 44100 Hz real int16 with two channels through Receiver(sample_rate=44100, resample=True, audio_source=chunks): the
    complete-cycle pass delivers every message of decode_stream once per channel, with its channel and band"""
    x, offs, _ = rcases.recipe(0, 44100, False)
    rate, t_first = 44100, 15.0 * 1000
    want = [set(texts(lst)) for lst in rx.decode_stream(x, rate, dial_offsets_hz=offs, resample=True)]
    cs = _t.strftime("%y%m%d_%H%M%S", _t.gmtime(t_first))
    vt, lock, got, box = [t_first], threading.Lock(), [], []

    def source():
        # the source delivers 15 s in a fraction of a second, so it waits for the daemon to take the passes that have fallen due
        for at in range(0, len(x), 30011):
            with lock:
                vt[0] = t_first + min(at + 30011, len(x)) / rate
            yield x[at:at + 30011]
            while box and box[0].wide_in._ready and box[0].thread_error is None and box[0]._thread.is_alive():
                _t.sleep(0.0005)

    live = Receiver("x", got.append, time_source=lambda: vt[0], sleep=lambda dt: _t.sleep(0.002), audio_source=source(), sample_rate=rate,
                    dial_offsets_hz=offs, bands=BANDS, t_first=t_first, resample=True, early_decode_hop=None)
    box.append(live)
    try:
        assert live._thread is not None and live.wide_in.n_channels == 2 and live.wide_in.rat and not live.wide_in.wide
        deadline = _t.time() + 120
        while not (live.wide_in.source_exhausted and not live.wide_in._ready) and live.thread_error is None and _t.time() < deadline:
            _t.sleep(0.02)
    finally:
        live.stop()
    assert live.thread_error is None and live.wide_in.source_exhausted and live.wide_in.n_pushed == len(x)
    for j in range(2):
        lst = [d for d in got if d["channel"] == j and not d["early"]]
        assert all(d["band"] == BANDS[j] and d["cyclestart_string"] == cs and 0.0 < d["fHz"] < 3000.0 for d in lst)
        t = texts(lst)
        print(f"live rat channel {j}: {len(t)} messages")
        assert len(set(t)) == len(t) and set(t) == want[j] and len(t) >= 5


# ---- refusals
def test_refusals_and_untouched_default_paths(handle):
    audio = np.stack([load_golden(n)[0] for n in ("test_08", "synth_000000")])
    before = handle.decode_batch(audio)
    # the other two paths on inputs of their own, before anything rational has run on the handle
    iq48, offs48, _ = cases.recipe(0, 4)
    xw = np.random.Generator(np.random.Philox(key=11)).integers(0, 256, size=(24000, 2)).astype(np.uint8)
    handle.ddc(iq48[None], ddc.IQ_I16, 48000, [0, 0], offs48)
    plain = handle.download_audio(handle.staging_ptr(), 2)
    handle.ddc_wide(xw, dw.IQ_U8, 240000, dials(240000))
    wide = handle.download_audio(handle.staging_ptr(), 3)
    L, h = handle._L, handle._h
    rate = 44100
    x = np.zeros(rate + 1, np.int16)
    f, fm = np.array(dials(rate) + [0.0]), np.zeros(4)
    src = np.zeros(3, np.int32)

    def err():
        return L.ft8rx_last_error(h).decode()

    def call(kind=dr.REAL_I16, rate=rate, n=1000, n_out=3):
        return L.ft8rx_ddc_rat_host(h, x.ctypes.data, kind, rate, n, n_out, f.ctypes.data, 1.0, fm.ctypes.data)

    def open_(kind=dr.REAL_I16, rate=rate, n_out=3, n_origin=0):
        return L.ft8rx_ddc_rat_stream_open(h, kind, rate, n_out, f.ctypes.data, 1.0, n_origin, 0, None)

    assert call() == 0
    # nothing is open yet
    assert L.ft8rx_ddc_rat_stream_push(h, x.ctypes.data, 1000, 0, None) == -1 and "no rational stream is open" in err()
    assert L.ft8rx_ddc_rat_stream_read_mid(h, 0, 10, fm.ctypes.data) == -1 and "no rational stream is open" in err()
    assert L.ft8rx_ddc_rat_stream_close(h) == -1
    with pytest.raises(_lib.Ft8rxError, match="no rational stream is open"):
        handle.ddc_rat_stream_push(x[:100])
    for fn in (call, open_):
        for kw, word in (({"kind": 4}, "kind"), ({"kind": 16}, "kind"), ({"kind": 17}, "kind"), ({"kind": 20}, "kind"), ({"kind": -1}, "kind"),
                         ({"rate": 900001}, "rate_hz"), ({"rate": 12500000}, "rate_hz"), ({"rate": 25000000}, "rate_hz"), ({"rate": 15999}, "rate_hz"),
                         ({"rate": 48000}, "rate_hz"), ({"rate": 240000}, "rate_hz"), ({"rate": 2400000}, "rate_hz"),
                         ({"n_out": 4}, "n_out"), ({"n_out": 0}, "n_out")):
            assert fn(**kw) == -1 and word in err(), (fn.__name__, kw, err())
        f[1] = 0.5 * rate
        assert fn() == -1 and "f_dial_hz[1]" in err()
        f[1] = -0.5 * rate - 1.0
        assert fn() == -1 and "f_dial_hz[1]" in err()
        f[1] = dials(rate)[1]
    assert call(n=15 * rate + 1) == -1 and "n_samples" in err()
    assert L.ft8rx_ddc_rat(h, None, dr.REAL_I16, rate, 1000, 3, f.ctypes.data, 1.0, None, None, None) == -1 and "d_in" in err()
    grid = origin_grid(rate)
    assert grid == 18522 and origin_grid(10000000) == 840000
    for n_origin in (1, 147, grid - 1, grid // 2, grid + 147, 2 ** 52 // grid * grid + grid):
        assert open_(n_origin=n_origin) == -1 and "n_origin" in err()
    with pytest.raises(_lib.Ft8rxError, match="kind"):
        handle.ddc_rat(x[:100], 7, rate, [0.0])
    # one stream per handle; while the rational stream is open the other stream opens and both one-shots behind a pre-stage are refused
    assert open_(n_origin=3 * grid) == 0
    assert open_() == -1 and "open on this handle already" in err()
    assert L.ft8rx_ddc_stream_open(h, ddc.IQ_I16, 48000, 1, 3, src.ctypes.data, f.ctypes.data, 1.0, 0, 0, None) == -1 and "rational stream is open" in err()
    assert L.ft8rx_ddc_stream_push(h, x.ctypes.data, 100, 0, None) == -1 and "rational stream" in err()
    assert L.ft8rx_ddc_stream_close(h) == -1 and "rational stream" in err()
    fw = np.array(dials(240000))
    assert L.ft8rx_ddc_wide_stream_open(h, dw.IQ_I16, 240000, 3, fw.ctypes.data, 1.0, 0, 0, None) == -1 and "rational stream is open" in err()
    assert L.ft8rx_ddc_wide_host(h, xw.ctypes.data, dw.IQ_U8, 240000, 1000, 3, fw.ctypes.data, 1.0, None) == -1 and "rational stream is open" in err()
    assert call() == -1 and "rational stream is open" in err()
    handle.ddc(iq48[None], ddc.IQ_I16, 48000, [0, 0], offs48)                          # ft8rx_ddc is not refused
    for n_new in (0, rate + 1):
        assert L.ft8rx_ddc_rat_stream_push(h, x.ctypes.data, n_new, 0, None) == -1 and "n_new" in err()
    assert L.ft8rx_ddc_rat_stream_push(h, None, 100, 0, None) == -1 and "in is NULL" in err()
    m = np.zeros(1, np.uint64)
    m_origin = 3 * grid * 12000 // rate
    assert L.ft8rx_ddc_rat_stream_push(h, x.ctypes.data, rate, 0, m.ctypes.data) == 0 and m_origin < int(m[0]) <= m_origin + 12000
    assert L.ft8rx_ddc_rat_stream_read_mid(h, 0, 10, fm.ctypes.data) == -1 and "not all held" in err()
    mid = handle.decode_batch(audio)                                                 # a decode while the stream is open
    assert L.ft8rx_ddc_rat_stream_close(h) == 0
    assert L.ft8rx_ddc_rat_stream_push(h, x.ctypes.data, 1000, 0, None) == -1 and "no rational stream is open" in err()
    assert open_() == 0 and L.ft8rx_ddc_rat_stream_close(h) == 0                     # close, then open again
    # ... and the other way round: not beside a plain or a wide stream, nor the one-shot beside a wide stream
    f48 = np.zeros(3)
    assert L.ft8rx_ddc_stream_open(h, ddc.IQ_I16, 48000, 1, 3, src.ctypes.data, f48.ctypes.data, 1.0, 0, 0, None) == 0
    assert open_() == -1 and "a stream is open on this handle already" in err()
    assert L.ft8rx_ddc_stream_close(h) == 0
    assert L.ft8rx_ddc_wide_stream_open(h, dw.IQ_I16, 240000, 3, fw.ctypes.data, 1.0, 0, 0, None) == 0
    assert open_() == -1 and "wide stream is open" in err()
    assert call() == -1 and "wide stream is open" in err()
    assert L.ft8rx_ddc_wide_stream_close(h) == 0
    assert call() == 0                                                               # and a good call still runs
    # after the rational one-shots: the other two paths give the bytes they gave before, and so does a decode
    handle.ddc(iq48[None], ddc.IQ_I16, 48000, [0, 0], offs48)
    assert handle.download_audio(handle.staging_ptr(), 2).tobytes() == plain.tobytes() and np.abs(plain).max() > 1000
    handle.ddc_wide(xw, dw.IQ_U8, 240000, dials(240000))
    assert handle.download_audio(handle.staging_ptr(), 3).tobytes() == wide.tobytes() and np.abs(wide).max() > 1000
    after = handle.decode_batch(audio)
    for other in (mid, after):
        assert before[1].tobytes() == other[1].tobytes() and before[3].tobytes() == other[3].tobytes() and before[1].min() > 0
        for fr in range(2):
            nc, ne = int(before[1][fr]), min(int(before[3][fr]), _lib.EVENT_CAP)
            assert before[0][fr, :nc].tobytes() == other[0][fr, :nc].tobytes()
            assert sorted(e.tobytes() for e in before[2][fr, :ne]) == sorted(e.tobytes() for e in other[2][fr, :ne])
