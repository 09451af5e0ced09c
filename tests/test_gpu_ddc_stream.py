"""The streaming down-converter on the GPU (ft8rx_ddc_stream_*): its first cycle against the one-shot kernel
byte for byte, chunk invariance across the input ring's wrap, its float64 twin (pyft8_amd/ddc.py: reference_stream) across a cycle
boundary and across the 2^32 phase wrap, the gather into frames, the live receiver on wide input end to end, and the refusals.

Error of the float32 output against the twin, full-scale random IQ int16 input, three channels (counts; measured on an MI355X, see
DESIGN.md section 16.1), printed by test_twin_*:
  cycle boundary, 24 kHz, outputs [177984, 182016):  max 0.021, rms 0.0025 (bound 3.58)
  phase wrap, 192 kHz, n_origin 4294934784:          max 0.0093, rms 0.00098 (bound 5.58)"""

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import ddc_stream_cases as live
from conftest import load_golden
from pyft8_amd import _lib, ddc
from pyft8_amd.receiver import Receiver

pytestmark = pytest.mark.gpu

NSAMP = 180000
TILE = 1008
SRC = [1, 0, 1]
KINDS_RATES = [(k, 12000 * D) for k in range(4) for D in (1, 2, 4, 8, 16) if not (k == ddc.REAL_I16 and D == 1)]


def dials(rate):
    """those of tests/test_gpu_ddc.py: negative and within 1 kHz of -rate/2; positive; within 1 kHz of +rate/2 (fc = dial + 3000 wraps)"""
    return [-0.5 * rate + 400.5, 0.11 * rate + 33.3, 0.5 * rate - 700.25]


def bound(kind, rate, gain, xmax):
    """The project's bound (tests/test_gpu_ddc.py): (n_macs + 16) 2^-23 G max|x|, n_macs = len(h1) + len(h2) multiply-adds on the path
    into one output, G = gain g sum|h1| sum|h2|.  Each float32 operation adds at most 2^-24 of the magnitudes summed so far; the 16
    covers the two rounded phasor tables, their product, the mixing product and the final scaling."""
    h1, h2 = ddc.taps(rate, 1), ddc.taps(rate, 2)
    g = 1.0 if ddc.is_iq(kind) else 2.0
    G = gain * g * (np.abs(h1.astype(np.float64)).sum() if len(h1) else 1.0) * np.abs(h2.astype(np.float64)).sum()
    return (len(h1) + len(h2) + 16) * 2.0 ** -23 * G * xmax


_data = {}


def iq(n, key):
    """Two streams of full-scale random IQ int16 [2, n, 2], the corners of the range at both ends"""
    if (n, key) not in _data:
        rng = np.random.Generator(np.random.Philox(key=0x57EA + key))
        x = rng.integers(-32768, 32768, size=(2, n, 2), dtype=np.int64).astype(np.int16)
        x[0, :3], x[1, -3:] = [[32767, -32768]] * 3, [[-32768, -32768]] * 3
        x.setflags(write=False)
        _data[(n, key)] = x
    return _data[(n, key)]


def of_kind(x, kind):
    if kind == ddc.IQ_I16:
        return x
    if kind == ddc.REAL_I16:
        return np.ascontiguousarray(x[:, :, 0])
    f = x.astype(np.float32) * np.float32(0.375)
    return f if kind == ddc.IQ_F32 else np.ascontiguousarray(f[:, :, 0])


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle(device=0, max_frames=3)
    yield h
    h.close()


@pytest.fixture()
def stream(handle):
    """open(...) opens the handle's stream; it is closed after the test whatever happened"""
    def open_(kind, rate, **kw):
        return handle.ddc_stream_open(kind, rate, 2, SRC, dials(rate), keep_f32=True, **kw)
    yield open_
    if handle._ds is not None:
        handle.ddc_stream_close()


@pytest.mark.parametrize("kind,rate", KINDS_RATES, ids=[f"{ddc.KIND_NAMES[k].replace(' ', '_')}-{r}" for k, r in KINDS_RATES])
def test_first_cycle_is_the_one_shot(handle, stream, kind, rate):
    """5000 D samples pushed, the same samples through ft8rx_ddc: the four complete tiles (m < 4032, every output whose inputs lie
    inside the pushed samples) are the same bytes, int16 and float32"""
    D = rate // 12000
    x = of_kind(iq(5000 * D, D), kind)
    fm1, y1 = handle.ddc(x, kind, rate, SRC, dials(rate), want_float=True)
    a1 = handle.download_audio(handle.staging_ptr(), 3)
    fm = stream(kind, rate)
    assert handle.ddc_stream_push(x) == 4 * TILE
    a, y = handle.ddc_stream_read(0, 4 * TILE, want_float=True)
    assert np.array_equal(fm, fm1)
    assert np.abs(y).max() > 1000                                                     # a real signal came out
    assert y.tobytes() == y1[:, :4 * TILE].tobytes()
    assert a.tobytes() == a1[:, :4 * TILE].tobytes()


def chunks_of(total, lens):
    out, i = [], 0
    while sum(out) < total:
        out.append(min(lens[i % len(lens)], total - sum(out)))
        i += 1
    return out


@pytest.mark.parametrize("rate", [24000, 192000])
def test_chunk_invariance(handle, stream, rate):
    """One stream set pushed in 1-s chunks and in chunks cycling through 1, 479, 480 D, 7 D + 3, more samples than the input ring holds
    (so it wraps), with a one-shot ft8rx_ddc on the same handle in the middle: every output is the same bytes"""
    D = rate // 12000
    total = rate + rate // 2 + 77
    x = iq(total, 100 + D)
    got = []
    for lens in ([rate], [1, 479, 480 * D, 7 * D + 3]):
        stream(ddc.IQ_I16, rate)
        assert total > handle.ddc_stream_info()["in_capacity"] >= rate
        at, m = 0, 0
        for i, n in enumerate(chunks_of(total, lens)):
            m_new = handle.ddc_stream_push(x[:, at:at + n])
            assert m_new >= m and m_new % TILE == 0
            at, m = at + n, m_new
            if at >= total // 2 > at - n and len(lens) > 1:                           # the one-shot uses nothing of the stream
                handle.ddc(iq(5000 * D, D), ddc.IQ_I16, rate, SRC, dials(rate))
        info = handle.ddc_stream_info()
        assert info["n_pushed"] == total and info["m_produced"] == m and info["out_capacity"] == 2 * NSAMP
        assert m >= (total // D) - 2 * TILE - 100                                       # at most a tile and the filters' reach behind
        got.append(handle.ddc_stream_read(0, m, want_float=True))
        handle.ddc_stream_close()
    assert got[0][0].shape == got[1][0].shape and np.abs(got[0][1]).max() > 1000
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()


def against_twin(handle, what, rate, x, n_origin, m_lo, m_hi):
    y = handle.ddc_stream_read(m_lo, m_hi - m_lo, want_float=True)[1]
    xmax = float(np.sqrt((x.astype(np.float64) ** 2).sum(axis=2)).max())
    lim = bound(ddc.IQ_I16, rate, 1.0, xmax)
    worst = 0.0
    for j, (s, f) in enumerate(zip(SRC, dials(rate))):
        ref = ddc.reference_stream(x[s], ddc.IQ_I16, rate, f, m_lo, m_hi, n_origin=n_origin)
        err = y[j].astype(np.float64) - ref
        print(f"ddc stream twin {what}, channel {j}: max |err| {np.abs(err).max():.5f}, rms {np.sqrt((err ** 2).mean()):.6f} counts, "
              f"bound {lim:.4f}, rms of y {y[j].std():.1f}")
        assert y[j].std() > 1000
        worst = max(worst, np.abs(err).max())
    assert worst <= lim


def test_twin_across_a_cycle_boundary(handle, stream):
    rate = 24000
    x = iq(16 * rate, 7)
    stream(ddc.IQ_I16, rate)
    for k in range(16):
        m = handle.ddc_stream_push(x[:, k * rate:(k + 1) * rate])
    assert m >= NSAMP + 2016
    against_twin(handle, "cycle boundary 24 kHz", rate, x, 0, NSAMP - 2016, NSAMP + 2016)


def test_twin_across_the_phase_wrap(handle, stream):
    """n_origin = the largest multiple of 1008 D below 2^32 - 2 x 1008 D at D = 16: n passes 2^32 inside the tiles produced"""
    rate, D = 192000, 16
    n_origin = (2 ** 32 - 2 * TILE * D - 1) // (TILE * D) * (TILE * D)
    assert n_origin % (TILE * D) == 0 and n_origin < 2 ** 32 - 2 * TILE * D <= n_origin + TILE * D
    x = iq(6 * TILE * D, 9)
    stream(ddc.IQ_I16, rate, n_origin=n_origin)
    handle.ddc_stream_push(x[:, :50001])
    m = handle.ddc_stream_push(x[:, 50001:])
    m0 = n_origin // D
    assert m - m0 >= 4 * TILE and (m0 + 4 * TILE) * D > 2 ** 32
    against_twin(handle, "phase wrap 192 kHz", rate, x, n_origin, m0, m0 + 4 * TILE)


def test_gather(handle, stream):
    """ft8rx_ddc_stream_frame against the ring's own bytes: odd and negative m_first, n_have below a frame, a range that wraps the
    output ring, a range that has left it"""
    rate = 24000
    x = iq(rate, 11)
    stream(ddc.IQ_I16, rate)
    for _ in range(3):
        m = handle.ddc_stream_push(x)

    def frames(m_first, n_have):
        handle.ddc_stream_frame(m_first, n_have)
        got = handle.download_audio(handle.staging_ptr(), 3)
        want = np.zeros((3, NSAMP), np.int16)
        lo, hi = max(m_first, 0), min(m_first + n_have, m)
        if hi > lo:
            want[:, lo - m_first:hi - m_first] = handle.ddc_stream_read(lo, hi - lo)
        assert got.tobytes() == want.tobytes(), (m_first, n_have)
        return got

    assert 30000 < m < 36000
    a = frames(1001, NSAMP)                                                            # odd; a zero tail beyond the outputs produced
    assert a[:, :m - 1001].std() > 1000 and not a[:, m - 1001:].any()
    a = frames(-6001, NSAMP)                                                           # before the origin: a zero head
    assert not a[:, :6001].any() and a[:, 6001:6001 + m].std() > 1000
    a = frames(2000, 5000)                                                             # n_have < 180000: a zero tail
    assert a[:, :5000].std() > 1000 and not a[:, 5000:].any()
    frames(-NSAMP - 5, NSAMP)                                                          # nothing of it exists: zeros
    for _ in range(29):
        m = handle.ddc_stream_push(x)
    assert 2 * NSAMP + 20000 < m < 2 * NSAMP + 24000
    a = frames(2 * NSAMP - 9999, 30000)                                                # wraps the output ring
    assert a[:, :30000].std() > 1000
    frames(m - 2 * NSAMP, NSAMP)                                                       # the oldest outputs the ring holds
    with pytest.raises(_lib.Ft8rxError, match="left the ring"):
        handle.ddc_stream_frame(m - 2 * NSAMP - 1, NSAMP)
    with pytest.raises(_lib.Ft8rxError, match="left the ring"):
        handle.ddc_stream_frame(-6000, NSAMP)
    with pytest.raises(_lib.Ft8rxError, match="n_have"):
        handle.ddc_stream_frame(m - 1000, NSAMP + 1)


def test_refusals_and_untouched_default_path(handle):
    audio = np.stack([load_golden(n)[0] for n in ("test_08", "synth_000000")])
    before = handle.decode_batch(audio)
    L, h = handle._L, handle._h
    x = np.zeros((2, 48000, 2), np.int16)
    src, f = np.array(SRC, np.int32), np.array(dials(48000))

    def err():
        return L.ft8rx_last_error(h).decode()

    def open_(kind=ddc.IQ_I16, rate=48000, n_streams=2, n_out=3, n_origin=0):
        return L.ft8rx_ddc_stream_open(h, kind, rate, n_streams, n_out, src.ctypes.data, f.ctypes.data, 1.0, n_origin, 0, None)

    # nothing is open yet
    assert L.ft8rx_ddc_stream_push(h, x.ctypes.data, 1000, 0, None) == -1 and "no stream is open" in err()
    assert L.ft8rx_ddc_stream_frame(h, 0, NSAMP, None) == -1 and "no stream is open" in err()
    assert L.ft8rx_ddc_stream_info(h, None, None, None, None) == -1 and L.ft8rx_ddc_stream_close(h) == -1
    with pytest.raises(_lib.Ft8rxError, match="no stream is open"):
        handle.ddc_stream_push(x[:, :100])
    # what ft8rx_ddc refuses, and an origin off the tile grid
    for kw, word in (({"kind": 4}, "kind"), ({"rate": 44100}, "rate_hz"), ({"kind": ddc.REAL_I16, "rate": 12000}, "real int16"),
                     ({"n_out": 4}, "n_out"), ({"n_out": 0}, "n_out"), ({"n_streams": 1}, "src[0]"), ({"n_origin": 1008 * 4 + 4}, "n_origin"),
                     ({"n_origin": 1008}, "n_origin"), ({"n_origin": 1008 * 2, "rate": 96000}, "n_origin")):
        assert open_(**kw) == -1 and word in err(), (kw, err())
    f[0] = 24000.0
    assert open_() == -1 and "f_dial_hz[0]" in err()
    f[0] = dials(48000)[0]
    assert open_(n_origin=1008 * 4 * 5) == 0
    assert open_() == -1 and "open on this handle already" in err()
    for n_new in (0, 48001):
        assert L.ft8rx_ddc_stream_push(h, x.ctypes.data, n_new, 0, None) == -1 and "n_new" in err()
    assert L.ft8rx_ddc_stream_push(h, None, 100, 0, None) == -1 and "in is NULL" in err()
    m = np.zeros(1, np.uint64)
    assert L.ft8rx_ddc_stream_push(h, x.ctypes.data, 48000, 0, m.ctypes.data) == 0 and 1008 * 5 < int(m[0]) <= 1008 * 5 + 12000
    mid = handle.decode_batch(audio)                                                 # a decode while the stream is open
    assert L.ft8rx_ddc_stream_close(h) == 0
    assert L.ft8rx_ddc_stream_push(h, x.ctypes.data, 1000, 0, None) == -1 and "no stream is open" in err()
    assert open_() == 0 and L.ft8rx_ddc_stream_close(h) == 0                         # close, then open again
    after = handle.decode_batch(audio)
    # (rows beyond a frame's counts are whatever the result slot held, and the event log is written in arrival order: compare the
    # records the counts cover and the events as a set)
    for other in (mid, after):
        assert before[1].tobytes() == other[1].tobytes() and before[3].tobytes() == other[3].tobytes() and before[1].min() > 0
        for fr in range(2):
            nc, ne = int(before[1][fr]), min(int(before[3][fr]), _lib.EVENT_CAP)
            assert before[0][fr, :nc].tobytes() == other[0][fr, :nc].tobytes()
            assert sorted(e.tobytes() for e in before[2][fr, :ne]) == sorted(e.tobytes() for e in other[2][fr, :ne])


def live_chunks(x):
    """The stream in chunks of 1920 and 1000 samples alternately -> (chunk, samples pushed once it is in)"""
    at, i = 0, 0
    while at < len(x):
        n = (1920, 1000)[i % 2]
        yield x[at:at + n], min(at + n, len(x))
        at, i = at + n, i + 1


def test_live_end_to_end():
    """Two cycles of 48 kHz IQ int16 with two channels (tests/ddc_stream_cases.py; the inputs are checked against the oracle by
    tests/test_ddc_stream.py) through Receiver(sample_rate=...): pushed directly with a poll() after every chunk, then once more from an
    iterator with the daemon thread.  Per cycle and channel the six transmitted texts arrive, none twice, with the right channel, band
    and cycle, some of them early, before the cycle's last sample has been pushed; decode_stream on each cycle's block gives the same."""
    import threading
    import time as _t
    x, offs, rate = live.stream(), live.offsets(), live.RATE
    t_first = 15.0 * 1000
    per_cycle = NSAMP * rate // 12000
    cs = [_t.strftime("%y%m%d_%H%M%S", _t.gmtime(t_first + 15 * c)) for c in range(2)]
    want = {(c, j): live.messages(live.PLAN[c][j])[0] for c in range(2) for j in range(2)}
    vt, pushed, got = [t_first], [0], []
    rx = Receiver("x", lambda d: got.append((pushed[0], d)), time_source=lambda: vt[0], sample_rate=rate, iq=True, dial_offsets_hz=offs,
                  bands=live.BANDS, t_first=t_first)
    try:
        assert rx._thread is None and rx.wide_in.n_channels == 2
        returned = []
        for chunk, n in live_chunks(x):
            pushed[0], vt[0] = n, t_first + n / rate
            rx.wide_in.push(chunk)
            returned += rx.poll()
        rx.wide_in.flush()                                                            # the source ends with the second cycle
        returned += rx.poll()
        assert rx._live.max_frames == 2 and rx._live.ddc_stream_info()["n_pushed"] >= len(x)
    finally:
        rx.stop()
    assert returned == [d for _, d in got]                                            # poll() returns what on_message saw
    by = {k: [] for k in want}
    for n, d in got:
        c = cs.index(d["cyclestart_string"])
        assert d["band"] == live.BANDS[d["channel"]] and d["their_tx_cycle"] == c % 2 and 0.0 < d["fHz"] < 3000.0
        by[(c, d["channel"])].append((n, d))
    for (c, j), lst in by.items():
        texts = [" ".join(d["msg_tuple"]) for _, d in lst]
        print(f"live cycle {c} channel {j}: {len(texts)} messages, {sum(d['early'] for _, d in lst)} early")
        assert len(set(texts)) == len(texts) and set(texts) == want[(c, j)], (c, j, sorted(texts))
        assert all(n < per_cycle * (c + 1) for n, d in lst if d["early"]) and all(n >= per_cycle * (c + 1) for n, d in lst if not d["early"])
    for c in range(2):
        assert any(d["early"] for j in range(2) for _, d in by[(c, j)])
    # control: each cycle's block alone through decode_stream
    ctl = Receiver("", None, max_frames=2)
    for c in range(2):
        res = ctl.decode_stream(x[None, per_cycle * c:per_cycle * (c + 1)], rate, iq=True, dial_offsets_hz=offs)
        for j in range(2):
            assert {" ".join(d["msg_tuple"]) for d in res[j]} == want[(c, j)], (c, j)
    ctl.close()

    # the same stream from an iterator: the constructor opens the source and starts the daemon (virtual clock and sleep seams)
    lock, got2, box = threading.Lock(), [], []

    def source():
        # a live source delivers 15 s in 15 s; this one delivers them in a fraction of a second, so it waits for the daemon to take the
        # passes that have fallen due (the output ring holds two cycles: a pass that is run later than that is refused)
        for chunk, n in live_chunks(x):
            with lock:
                vt[0] = t_first + n / rate
            yield chunk
            while box and box[0].wide_in._ready and box[0].thread_error is None and box[0]._thread.is_alive():
                _t.sleep(0.0005)

    rx = Receiver("x", got2.append, time_source=lambda: vt[0], sleep=lambda dt: _t.sleep(0.002), audio_source=source(), sample_rate=rate,
                  iq=True, dial_offsets_hz=offs, bands=live.BANDS, t_first=t_first)
    box.append(rx)
    try:
        assert rx._thread is not None and rx._thread.is_alive()
        deadline = _t.time() + 120
        while not (rx.wide_in.source_exhausted and not rx.wide_in._ready) and rx.thread_error is None and _t.time() < deadline:
            _t.sleep(0.02)
    finally:
        rx.stop()                                                                     # joins the daemon: the pass it is in completes
    assert rx.thread_error is None and rx.wide_in.source_exhausted

    def key(d):
        return (d["cyclestart_string"], d["channel"], d["band"], " ".join(d["msg_tuple"]))
    assert sorted(key(d) for d in got2) == sorted(key(d) for _, d in got)
    assert any(d["early"] for d in got2)
