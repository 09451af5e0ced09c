"""ft8rx_pan* (csrc/kernels/pan.hpp) against its float64 twin pyft8_amd/pan.py on the crafted streams of
tests/pan_cases.py: accuracy for every kind and size, crafted windows that fix the bin order and the window indexing, the stream byte
for byte against the one-shot in every chunking, the statistics, the input forms, independence of the other streams, and Receiver /
WideIn with panorama=.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import blank_in_cases as bcases
import pan_cases as cases
from pyft8_amd import _lib, pan
from pyft8_amd import blank_in as bi
from pyft8_amd import kinds as K
from pyft8_amd.receiver import Receiver

pytestmark = pytest.mark.gpu
IDS = [cases.KIND_IDS[k] for k in cases.KINDS]
DEV = torch.device("cuda", 0)
# max_j |P - P64| / max_j P64 per row over the 72 cases of test_accuracy_against_the_twin: measured 2.12e-7 at the worst (IQ float32,
# N = 8192, A = 1; profiles/pan_notes.md), asserted at 4 x that rounded up to one digit.  Rounding alone cannot exceed
# (A + 64) 2^-23 (a float32 sum of A non-negative terms to first order, log2 N FFT passes with generous room): the other assertion.
BOUND = 9e-7


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle(max_frames=2)
    yield h
    h.close()


def _to_device(a):
    d = torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)
    torch.cuda.synchronize(DEV)
    return d


def _err(got, want):
    """max_j |P - P64| / max_j P64 per row"""
    return np.abs(got.astype(np.float64) - want).max(axis=1) / want.max(axis=1)


@pytest.mark.parametrize("A", cases.AVGS)
@pytest.mark.parametrize("N", cases.SIZES)
@pytest.mark.parametrize("kind", cases.KINDS, ids=IDS)
def test_accuracy_against_the_twin(handle, kind, N, A):
    """(2 A + 1) N + 37 samples of seeded noise and two tones 60 dB apart: two rows (three at A = 1), the rest is dropped"""
    x = cases.noisy(kind, cases.accuracy_n(N, A))
    want, wstats = pan.reference(x, kind, N, A)
    got, stats = handle.pan(x, kind, N, A)
    assert got.shape == want.shape == ((2 * A + 1) // A, pan.bins(kind, N)) and got.dtype == np.float32
    e = _err(got, want)
    print(f"pan accuracy kind={cases.KIND_IDS[kind]} N={N} A={A}: {e.max():.3e}")
    assert e.max() <= (A + 64) * 2.0 ** -23, "beyond what rounding can do: a defect"
    assert e.max() <= BOUND
    assert (stats is None and wstats is None) or np.array_equal(stats, wstats)


def _close(got, want):
    assert got.shape == want.shape
    assert _err(got, want).max() <= BOUND, _err(got, want)


@pytest.mark.parametrize("N", [256, 2048])
def test_crafted_tones_fix_the_bin_order_the_shift_and_the_sign(handle, N):
    for kind in (K.IQ_I16, K.IQ_F32):
        for k0 in (7, -7, N // 2 - 1, -(N // 2)):
            x = cases.store(cases.tone(kind, 2 * N, k0 / N, 20000.0), kind)
            got, _ = handle.pan(x, kind, N, 2)
            _close(got, pan.reference(x, kind, N, 2)[0])
            assert int(np.argmax(got[0])) == N // 2 + k0
    for kind in (K.REAL_I16, K.REAL_F32):
        x = cases.store(cases.tone(kind, 2 * N, 9 / N, 20000.0), kind)
        got, _ = handle.pan(x, kind, N, 2)
        _close(got, pan.reference(x, kind, N, 2)[0])
        assert got.shape == (1, N // 2) and int(np.argmax(got[0])) == 9


def test_uint8_constants_fix_the_dc_bin_and_the_value_map(handle):
    N, A = 512, 3
    for code in (127, 128):
        x = np.full((N * A, 2), code, np.uint8)
        got, stats = handle.pan(x, K.WIDE_IQ_U8, N, A)
        _close(got, pan.reference(x, K.WIDE_IQ_U8, N, A)[0])
        dc = 2 * A * (128.0 * N / 2) ** 2
        assert abs(got[0, N // 2] - dc) <= 1e-6 * dc and abs(got[0, N // 2 + 1] - dc / 4) <= 1e-6 * dc and np.array_equal(stats, [[0, 1]])


@pytest.mark.parametrize("kind", [K.REAL_I16, K.IQ_F32, K.WIDE_IQ_I8], ids=["real_i16", "iq_f32", "iq_i8"])
def test_impulses_fix_the_window_indexing_and_silence_gives_zero_bytes(handle, kind):
    """an impulse at window position i0 gives the flat spectrum (w[i0] v)^2: position 0 gives exact zeros (w[0] = 0); then N / 2, the
    last sample of a window, the first sample of the next"""
    N, A = 256, 2
    w = pan.window(N).astype(np.float64)
    for at, where in ((0, 0), (N // 2, N // 2), (N - 1, N - 1), (N, 0), (3 * N + 5, 5)):
        x = np.zeros(K.shape(kind, 2 * N * A), K.DTYPE[kind])
        x[at] = 64
        got, _ = handle.pan(x, kind, N, A)
        want = pan.reference(x, kind, N, A)[0]
        row = at // (N * A)
        assert not got[1 - row].any()
        if where == 0:
            assert got.tobytes() == bytes(got.nbytes)
        else:
            _close(got[row:row + 1], want[row:row + 1])
            level = abs(w[where] * K.values(x, kind)[at]) ** 2
            assert np.allclose(got[row], level, rtol=1e-5)
    got, stats = handle.pan(np.zeros(K.shape(kind, N * A), K.DTYPE[kind]), kind, N, A)
    assert got.tobytes() == bytes(got.nbytes) and (stats is None or not stats.any())


def _predict(n_origin, n_end, N, A, n_rows):
    return pan.rows_done(n_origin, n_end, N, A)[1], pan.held(n_origin, n_end, N, A, n_rows)


@pytest.mark.parametrize("kind,n_origin,N,A", [(K.WIDE_IQ_U8, 0, 256, 3), (K.REAL_I16, 3 * 256 + 17, 256, 3), (K.IQ_F32, (1 << 40) + 255, 512, 2)],
                         ids=["iq_u8_origin_0", "real_i16_origin_785", "iq_f32_origin_2_40"])
def test_stream_in_every_chunking_is_the_one_shot_byte_for_byte(handle, kind, n_origin, N, A):
    """11 rows and a rest into a ring of 4: after every push info and rows_done are pan_ring.hpp's prediction, every row read when it
    is finished equals the one-shot's bytes (the one-shot on the samples from the first row's start), the ring drops the oldest rows,
    a dropped and a future row are refused by name, and nothing is allocated between open and close"""
    n_rows = 4
    x = cases.noisy(kind, 11 * N * A + 111)
    r_first = pan.rows_done(n_origin, n_origin, N, A)[0]
    skip = r_first * A * N - n_origin
    want, wstats = handle.pan(x[skip:], kind, N, A)
    assert len(want) >= 10 and _err(want, pan.reference(x, kind, N, A, n_origin=n_origin)[0]).max() <= BOUND
    cuts = dict(cases.chunkings(len(x), N, A, 2 * N * A + 3), at_once=[len(x)])
    for name, lengths in cuts.items():
        handle.pan_stream_open(kind, N, A, n_rows, n_origin=n_origin, max_push=len(x))
        try:
            handle.sync()
            free0 = torch.cuda.mem_get_info(DEV)[0]
            n_end, seen = n_origin, r_first
            for ch in cases.cut(x, lengths):
                _, r_done = handle.pan_stream_push(ch)
                n_end += len(ch)
                done, (r_lo, r_hi) = _predict(n_origin, n_end, N, A, n_rows)
                info = handle.pan_stream_info()
                assert r_done == done == info["rows_done"] == r_hi and info["r_lo"] == r_lo and info["n_pushed"] == n_end - n_origin, (name, info)
                lo = max(seen, r_lo)
                if r_done > lo:
                    rows, stats = handle.pan_stream_read(lo, r_done - lo)
                    assert rows.tobytes() == want[lo - r_first:r_done - r_first].tobytes(), (name, lo, r_done)
                    assert (stats is None and wstats is None) or np.array_equal(stats, wstats[lo - r_first:r_done - r_first])
                seen = r_done
            assert torch.cuda.mem_get_info(DEV)[0] == free0, name
            assert seen == r_first + len(want)
            # the ring wrapped: the last n_rows rows are there, in one read across the wrap; older and future rows are refused
            rows, _ = handle.pan_stream_read(seen - n_rows, n_rows)
            assert rows.tobytes() == want[len(want) - n_rows:].tobytes(), name
            with pytest.raises(_lib.Ft8rxError, match=rf"r_first.*holds the rows \[{seen - n_rows}, {seen}\)"):
                handle.pan_stream_read(seen - n_rows - 1, 1)
            with pytest.raises(_lib.Ft8rxError, match="holds the rows"):
                handle.pan_stream_read(seen, 1)
        finally:
            handle.pan_stream_close()


def test_more_rows_in_one_push_than_the_ring_holds(handle):
    """A = 1 and a ring of 3: a push of 10 windows runs in tiles of at most 3 windows and leaves the newest 3 rows"""
    kind, N = K.IQ_I16, 256
    x = cases.noisy(kind, 10 * N + 9)
    want, _ = handle.pan(x, kind, N, 1)
    handle.pan_stream_open(kind, N, 1, 3, max_push=len(x))
    try:
        assert handle.pan_stream_push(x)[1] == 10
        assert handle.pan_stream_read(7, 3)[0].tobytes() == want[7:].tobytes()
    finally:
        handle.pan_stream_close()


def test_destroy_releases_an_open_stream_and_the_one_shot_workspaces():
    """a handle closed with its panorama stream open leaves nothing behind: the third such handle ends where the second did (the
    first one may warm the runtime)"""
    x = cases.noisy(K.IQ_I16, 4 * 1024 + 7)
    free = []
    for _ in range(3):
        h = _lib.Handle(max_frames=1)
        h.pan(x, K.IQ_I16, 1024, 2)
        h.pan_stream_open(K.IQ_I16, 1024, 2, 64, max_push=1 << 20)
        assert h.pan_stream_push(x)[1] == 2
        h.close()
        torch.cuda.synchronize(DEV)
        free.append(torch.cuda.mem_get_info(DEV)[0])
    assert free[2] == free[1]


@pytest.mark.parametrize("kind", cases.KINDS, ids=IDS)
def test_statistics_match_the_twin_exactly(handle, kind):
    """rails and peaks planted in the first and the last sample of a row, on each component; float kinds report None"""
    N, A = 256, 3
    x = cases.noisy(kind, 3 * N * A, seed=3).copy()
    if not K.is_integer(kind):
        assert handle.pan(x, kind, N, A)[1] is None
        return
    info = np.iinfo(K.DTYPE[kind])
    flat = x.reshape(len(x), -1)
    np.clip(flat, info.min + 2, info.max - 2, out=flat)
    nc = flat.shape[1]
    flat[0, 0], flat[N * A - 1, nc - 1] = info.min, info.max                       # row 0: first and last sample
    flat[N * A, nc - 1], flat[2 * N * A - 1, 0] = info.max, info.max - 1            # row 1: one rail, one peak just below it
    flat[2 * N * A + 5, :] = info.min                                               # row 2: both components of one sample count once
    want = pan.reference(x, kind, N, A)[1]
    assert want[:, 0].tolist() == [2, 1, 1]
    assert np.array_equal(handle.pan(x, kind, N, A)[1], want)
    handle.pan_stream_open(kind, N, A, 8, max_push=1000)
    try:
        for at in range(0, len(x), 1000):
            handle.pan_stream_push(x[at:at + 1000])
        assert np.array_equal(handle.pan_stream_read(0, 3)[1], want)
    finally:
        handle.pan_stream_close()


@pytest.mark.parametrize("kind", [K.IQ_I16, K.WIDE_IQ_U8, K.IQ_F32, K.REAL_I16], ids=["iq_i16", "iq_u8", "iq_f32", "real_i16"])
def test_input_forms_give_the_same_bytes(handle, kind):
    """the device entry on a 16-byte aligned buffer, on one that is only component-aligned, and the host entry"""
    N, A = 1024, 2
    x = cases.noisy(kind, 2 * N * A + 5)
    raw = x.view(np.uint8).reshape(-1)
    cb = np.dtype(K.DTYPE[kind]).itemsize
    host, hstats = handle.pan(x, kind, N, A)
    d = _to_device(x)
    assert d.data_ptr() % 16 == 0
    got, stats = handle.pan(None, kind, N, A, d_ptr=d.data_ptr(), n=len(x))
    assert got.tobytes() == host.tobytes() and (stats is None or np.array_equal(stats, hstats))
    buf = np.zeros(raw.size + 64, np.uint8)
    buf[cb:cb + raw.size] = raw
    d = _to_device(buf)
    got, stats = handle.pan(None, kind, N, A, d_ptr=d.data_ptr() + cb, n=len(x))
    assert got.tobytes() == host.tobytes() and (stats is None or np.array_equal(stats, hstats))
    # a stream fed from that address
    handle.pan_stream_open(kind, N, A, 4, max_push=len(x))
    try:
        assert handle.pan_stream_push(None, d_ptr=d.data_ptr() + cb, n=len(x))[1] == 2
        assert handle.pan_stream_read(0, 2)[0].tobytes() == host.tobytes()
    finally:
        handle.pan_stream_close()


def test_other_streams_are_byte_identical_with_a_panorama_stream_open(handle):
    """the wide pre-decimator stream and the input blanker's released bytes, without a panorama stream, with one open beside them,
    and with the front end fed from the address the panorama push returns"""
    kind, rate, B = bi.WIDE_IQ_I16, 240000, 256
    x = bcases.case(kind, B)[0]
    x = np.concatenate([x] * (60000 // len(x) + 1))[:60000]
    chunks = cases.cut(x, [7000] * 8 + [4000])

    def run(mode):
        handle.ddc_wide_stream_open(kind, rate, [1000.0])
        handle.blank_in_stream_open(kind, B, max_push=7000)
        if mode:
            handle.pan_stream_open(kind, 256, 3, 8, max_push=8000)
        try:
            released, m = [], 0
            for i, ch in enumerate(chunks):
                d_out, _, n_out, y = handle.blank_in_stream_push(ch, finish=i == len(chunks) - 1, download=True)
                released.append(y)
                if n_out:
                    if mode == 2:
                        d_out = handle.pan_stream_push(None, d_ptr=d_out, n=n_out)[0]
                    elif mode == 1:
                        handle.pan_stream_push(ch)
                    m = handle.ddc_wide_stream_push(None, d_ptr=d_out, n=n_out)
            return np.concatenate(released).tobytes(), handle.ddc_stream_read(0, m).tobytes(), handle.blank_in_stream_info()["stats"].tolist()
        finally:
            if mode:
                handle.pan_stream_close()
            handle.blank_in_stream_close()
            handle.ddc_wide_stream_close()
    want = run(0)
    assert run(1) == want and run(2) == want and any(want[1])
    # ... and the plain and rational streams from the host while a panorama stream runs
    for name, args, push in (("ddc", (K.IQ_I16, 48000, 1, [0], [500.0]), np.stack([x[:20000]])), ("ddc_rat", (K.IQ_I16, 44100, [500.0]), x[:20000])):
        outs = []
        for with_pan in (False, True):
            getattr(handle, name + "_stream_open")(*args)
            if with_pan:
                handle.pan_stream_open(kind, 256, 3, 8, max_push=20000)
            try:
                if with_pan:
                    handle.pan_stream_push(x[:20000])
                m = getattr(handle, name + "_stream_push")(push)
                outs.append(handle.ddc_stream_read(0, m).tobytes())
            finally:
                if with_pan:
                    handle.pan_stream_close()
                getattr(handle, name + "_stream_close")()
        assert outs[0] == outs[1] and any(outs[0]), name


def test_refusals_name_the_argument(handle):
    L, h = handle._L, handle._h
    host = np.zeros(8192, np.int16)
    d = _to_device(host)
    p = d.data_ptr()

    def err():
        return L.ft8rx_last_error(h).decode()
    ok = (K.WIDE_IQ_U8, 4096, 256, 2)
    for i, v, name in ((0, 4, "kind"), (0, 20, "kind"), (0, -1, "kind"), (2, 128, "n_fft"), (2, 3000, "n_fft"), (2, 16384, "n_fft"), (3, 0, "n_avg"),
                       (3, 65537, "n_avg")):
        args = list(ok)
        args[i] = v
        assert L.ft8rx_pan(h, p, *args, None, None, None) == -1 and name in err(), (name, err())
        assert L.ft8rx_pan_host(h, host.ctypes.data, *args, None, None, None) == -1 and name in err()
        assert L.ft8rx_pan_stream_open(h, args[0], args[2], args[3], 8, 0, 1000) == -1 and name in err()
    assert L.ft8rx_pan(h, None, *ok, None, None, None) == -1 and "d_samples" in err()
    assert L.ft8rx_pan(h, p + 1, K.REAL_I16, 4096, 256, 2, None, None, None) == -1 and "d_samples" in err()
    assert L.ft8rx_pan_host(h, None, *ok, None, None, None) == -1 and "samples" in err()
    assert L.ft8rx_pan_stream_push(h, p, 10, 1, None, None) == -1 and "no panorama stream is open" in err()
    assert L.ft8rx_pan_stream_info(h, None, None, None, None) == -1 and L.ft8rx_pan_stream_close(h) == -1 and L.ft8rx_pan_stream_read(h, 0, 0, None, None) == -1
    assert L.ft8rx_pan_stream_open(h, K.IQ_I16, 256, 1, 0, 0, 1000) == -1 and "n_rows" in err()
    assert L.ft8rx_pan_stream_open(h, K.IQ_I16, 256, 1, 8, 0, 0) == -1 and "max_push" in err()
    assert L.ft8rx_pan_stream_open(h, K.IQ_I16, 256, 1, 8, 0, 1000) == 0
    try:
        assert L.ft8rx_pan_stream_open(h, K.IQ_I16, 256, 1, 8, 0, 1000) == -1 and "open on this handle already" in err()
        assert L.ft8rx_pan_stream_push(h, p, 1001, 1, None, None) == -1 and "n_new" in err()
        assert L.ft8rx_pan_stream_push(h, None, 10, 0, None, None) == -1 and "in is NULL" in err()
        assert L.ft8rx_pan_stream_push(h, p, 1000, 1, None, None) == 0 and L.ft8rx_pan_stream_push(h, None, 0, 0, None, None) == 0
        assert L.ft8rx_pan_stream_read(h, 0, 3, None, None) == 0 and L.ft8rx_pan_stream_read(h, 0, 4, None, None) == -1 and "n 4" in err()
    finally:
        assert L.ft8rx_pan_stream_close(h) == 0
    # the keyword: two streams
    rx = Receiver("", None, max_frames=2)
    try:
        with pytest.raises(_lib.Ft8rxError, match="panorama: 2 streams"):
            rx.decode_stream(np.zeros((2, 48000, 2), np.int16), 48000, iq=True, dial_offsets_hz=[0.0, 0.0], panorama=True)
        with pytest.raises(_lib.Ft8rxError, match="n_fft"):
            rx.decode_stream(np.zeros((48000, 2), np.int16), 48000, iq=True, panorama={"n_fft": 100})
    finally:
        rx.close()
    with pytest.raises(_lib.Ft8rxError, match="n_avg"):
        Receiver("", None, max_frames=1, panorama={"n_avg": 0})


# ---- Receiver
def _fields(d):
    return (" ".join(d["msg_tuple"]), d["their_snr"], d["fHz"], d["tsec"], d["decode_notes"])


@pytest.fixture(scope="module")
def cycle():
    """(the 240 kHz IQ int16 cycle with impulses of tests/blank_in_cases.py, its dial, the twin's blanked samples at the receiver's defaults)"""
    _, noisy, f_off, _, _ = bcases.benefit_recipe()[0]
    noisy = np.concatenate([noisy, noisy[:3600000 - len(noisy)]])
    return noisy, f_off, bi.reference(noisy, bi.WIDE_IQ_I16, 256)[0]


def _live(samples, f_off, **kw):
    """One live cycle through WideIn under a virtual clock, in uneven chunks with a poll() after each -> (messages, the panorama dict)"""
    rate, t_first = 240000, 15.0 * 1000
    vt, got = [t_first], []
    rx = Receiver("x", got.append, time_source=lambda: vt[0], sample_rate=rate, iq=True, dial_offsets_hz=[f_off], t_first=t_first,
                  early_decode_hop=320, waterfall=True, **kw)
    try:
        at, k = 0, 0
        while at < len(samples):
            n = (24000, 50001, 7, 240000, 3000)[k % 5]
            vt[0] = t_first + min(at + n, len(samples)) / rate
            rx.wide_in.push(samples[at:at + n])
            rx.poll()
            at, k = at + n, k + 1
        rx.wide_in.flush()
        rx.poll()
        p = rx.panorama
        t1 = rx.wide_in.panorama_time(1)
    finally:
        rx.stop()
    assert rx.thread_error is None
    return [_fields(d) + (d["early"],) for d in got], p, t1


def test_live_cycle_with_panorama_decodes_the_same_and_shows_the_blanked_stream(handle, cycle):
    noisy, f_off, blanked = cycle
    want, none, _ = _live(noisy, f_off, input_blanker=True)
    got, p, t1 = _live(noisy, f_off, input_blanker=True, panorama=True)
    assert none is None and got == want and len(want) >= 10
    rows, stats = handle.pan(blanked, bi.WIDE_IQ_I16, 2048, 19)
    assert p["n_fft"] == 2048 and p["n_avg"] == 19 and p["r_next"] == len(rows) == 92 and p["data"].shape == (256, 2048)
    assert p["data"][:92].tobytes() == rows.tobytes() and not p["data"][92:].any() and np.array_equal(p["stats"][:92], stats)
    assert abs(p["row_seconds"] - 2048 * 19 / 240000) < 1e-12 and t1 == 15000.0 + 2048 * 19 / 240000 and p["f_hz"][1024] == 0.0


def test_live_cycle_without_the_input_blanker_feeds_the_front_end_from_the_panorama_buffer(handle, cycle):
    """the chunk crosses once, into the panorama's work buffer, and the front end's device push reads it there: the same messages as
    the plain run, the raw stream's rows, a ring of 4 that wrapped"""
    noisy, f_off, _ = cycle
    plain, none, _ = _live(noisy, f_off)
    got, p, _ = _live(noisy, f_off, panorama={"n_fft": 1024, "period_s": 0.5, "rows": 4})
    assert none is None and got == plain and len(plain) >= 5
    rows, stats = handle.pan(noisy, bi.WIDE_IQ_I16, 1024, 117)
    assert p["n_avg"] == 117 and p["r_next"] == len(rows) == 30
    assert p["data"][np.arange(26, 30) % 4].tobytes() == rows[26:].tobytes() and np.array_equal(p["stats"][np.arange(26, 30) % 4], stats[26:])


def test_decode_stream_with_panorama(handle, cycle):
    noisy, f_off, blanked = cycle
    rx = Receiver("", None, max_frames=1)
    try:
        assert rx.panorama is None
        want = rx.decode_stream(noisy, 240000, iq=True, dial_offsets_hz=[f_off])
        got = rx.decode_stream(noisy, 240000, iq=True, dial_offsets_hz=[f_off], panorama={"n_fft": 4096, "n_avg": 10})
        assert [[_fields(d) for d in ch] for ch in got] == [[_fields(d) for d in ch] for ch in want] and len(want[0]) >= 5
        rows, stats = handle.pan(noisy, bi.WIDE_IQ_I16, 4096, 10)
        p = rx.panorama
        assert p["data"].tobytes() == rows.tobytes() and np.array_equal(p["stats"], stats) and p["r_next"] == len(rows) == 87
        # behind the input blanker it shows what the front end sees
        rx.decode_stream(noisy, 240000, iq=True, dial_offsets_hz=[f_off], input_blanker=True, panorama={"n_fft": 4096, "n_avg": 10})
        assert rx.panorama["data"].tobytes() == handle.pan(blanked, bi.WIDE_IQ_I16, 4096, 10)[0].tobytes()
        assert rx.panorama["data"].tobytes() != rows.tobytes()
    finally:
        rx.close()
