"""ft8rx_blank_in* (csrc/kernels/blank_in.hpp) against its numpy twin, bit for bit, on the crafted streams of
tests/blank_in_cases.py: the one-shot entries, the stream in every chunking, the chain into the three front ends on the device, and
Receiver / WideIn with input_blanker=.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import blank_in_cases as cases
from pyft8_amd import _lib, blanker
from pyft8_amd import blank_in as bi
from pyft8_amd import ddc_wide as dw
from pyft8_amd.receiver import Receiver

pytestmark = pytest.mark.gpu
IDS = [cases.KIND_IDS[k] for k in cases.KINDS]
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle(max_frames=2)
    yield h
    h.close()


def _to_device(a):
    d = torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)
    torch.cuda.synchronize(DEV)
    return d


def _cut(x, lengths):
    out, at = [], 0
    for c in lengths:
        out.append(x[at:at + c])
        at += c
    return out


@pytest.mark.parametrize("B", [256, 4096])
@pytest.mark.parametrize("kind", cases.KINDS, ids=IDS)
def test_one_shot_is_the_twin_bit_for_bit(handle, kind, B):
    """n = 7 B + 37: samples, stats and levels, in place on a caller's device buffer"""
    x, (y, stats, lv), _, _ = cases.case(kind, B)
    d = _to_device(x)
    ptr, n, gs, gl = handle.blank_in(None, kind, B, d_ptr=d.data_ptr(), n=len(x), want_levels=True)
    got = d.cpu().numpy()
    assert ptr == d.data_ptr() and n == len(x)
    assert np.array_equal(gl, lv), (gl, lv)
    assert np.array_equal(gs, stats), (gs, stats)
    assert got.tobytes() == y.tobytes(), np.flatnonzero((got != y).reshape(len(x), -1).any(axis=1))[:8]
    assert stats[0] >= 20 and got.tobytes() != x.tobytes()


@pytest.mark.parametrize("kind,args", [(bi.WIDE_REAL_I16, (2.0, 0, 0)), (bi.WIDE_IQ_U8, (5.5, 64, 64)), (bi.WIDE_IQ_I16, (8.0, 0, 64)),
                                       (bi.WIDE_IQ_I8, (4.0, 64, 0))], ids=["k2_g0_r0", "g64_r64", "g0_r64", "g64_r0"])
def test_one_shot_at_the_limits_of_guard_and_taper(handle, kind, args):
    x = cases.case(kind, 256)[0]
    k, G, R = args
    y, stats, lv = bi.reference(x, kind, 256, k, G, R)
    d = _to_device(x)
    _, _, gs, gl = handle.blank_in(None, kind, 256, int(round(256 * k)), G, R, d_ptr=d.data_ptr(), n=len(x), want_levels=True)
    assert np.array_equal(gl, lv) and np.array_equal(gs, stats) and d.cpu().numpy().tobytes() == y.tobytes()


@pytest.mark.parametrize("kind", [bi.WIDE_REAL_I16, bi.WIDE_IQ_I16, bi.WIDE_IQ_U8], ids=["real_i16", "iq_i16", "iq_u8"])
def test_where_the_result_goes(handle, kind):
    """Into d_out (the input keeps its bytes), through the host entry, queued only, and on a buffer that is only sample-aligned; the
    sentinel bytes around the samples stay"""
    B = 256
    x, (y, stats, _), _, _ = cases.case(kind, B)
    raw = x.view(np.uint8).reshape(-1)
    sb = raw.size // len(x)
    # d_out: another buffer, with a sentinel region behind the samples
    d_in = _to_device(x)
    out = np.full(raw.size + 4096, 0xA5, np.uint8)
    d_out = _to_device(out)
    ptr, n, gs = handle.blank_in(None, kind, B, d_ptr=d_in.data_ptr(), n=len(x), d_out=d_out.data_ptr())
    got = d_out.cpu().numpy()
    assert ptr == d_out.data_ptr() and np.array_equal(gs, stats)
    assert got[:raw.size].tobytes() == y.tobytes() and (got[raw.size:] == 0xA5).all() and d_in.cpu().numpy().tobytes() == x.tobytes()
    # the host entry: the handle's own buffer
    ptr, n, gs, back = handle.blank_in(x, kind, B, download=True)
    assert ptr != 0 and n == len(x) and np.array_equal(gs, stats) and back.tobytes() == y.tobytes()
    # queued only (no stats): the next call on the handle sees the result
    d = _to_device(x)
    assert handle.blank_in(None, kind, B, d_ptr=d.data_ptr(), n=len(x), want_stats=False)[2] is None
    handle.sync()
    assert d.cpu().numpy().tobytes() == y.tobytes()
    # one sample past a 16-byte boundary: the sample-by-sample path, the same bits, nothing outside the samples written
    buf = np.full(raw.size + 64, 0x5A, np.uint8)
    buf[sb:sb + raw.size] = raw
    d = _to_device(buf)
    assert d.data_ptr() % 16 == 0
    _, _, gs, gl = handle.blank_in(None, kind, B, d_ptr=d.data_ptr() + sb, n=len(x), want_levels=True)
    got = d.cpu().numpy()
    assert np.array_equal(gs, stats) and got[sb:sb + raw.size].tobytes() == y.tobytes()
    assert (got[:sb] == 0x5A).all() and (got[sb + raw.size:] == 0x5A).all()


@pytest.mark.parametrize("kind,n_origin", [(bi.WIDE_IQ_U8, 0), (bi.WIDE_REAL_I16, 3 * 256 + 17), (bi.WIDE_IQ_I16, (1 << 40) + 255)],
                         ids=["iq_u8_origin_0", "real_i16_origin_785", "iq_i16_origin_2_40"])
def test_stream_in_every_chunking_is_the_one_shot(handle, kind, n_origin):
    """1, B - 1, B, B + 1, 3 B + G + R, a mix and one max_push chunk: n_first / n_out are `released` after every push, the released
    samples concatenated are the twin's (and, from origin 0, the one-shot's), the stats too; nothing is allocated between open and
    close; the crafted stream has hit pairs on both sides of every block edge (a chunk boundary at chunk = B) and of every release
    boundary, and ends in a partial block"""
    B, G, R = 256, 6, 6
    x = cases.case(kind, B)[0]
    y, stats, _ = bi.reference(x, kind, B, n_origin=n_origin)
    if n_origin == 0:
        assert y.tobytes() == cases.case(kind, B)[1][0].tobytes()
    for name, cut in cases.chunkings(len(x), B, G, R).items():
        handle.blank_in_stream_open(kind, B, n_origin=n_origin, max_push=len(x))
        try:
            handle.sync()
            free0 = torch.cuda.mem_get_info(DEV)[0]
            parts, n_end, first_free = [], n_origin, n_origin
            for i, ch in enumerate(_cut(x, cut)):
                fin = i == len(cut) - 1 and name != "mix"
                _, n_first, n_out, got = handle.blank_in_stream_push(ch, finish=fin, download=True)
                n_end += len(ch)
                want_end = n_end if fin else bi.released(n_origin, n_end, B, G, R)
                assert n_first == first_free and n_first + n_out == want_end, (name, i, n_first, n_out, want_end)
                first_free = want_end
                parts.append(got)
            if name == "mix":                              # finish as a push of its own, with no samples
                _, n_first, n_out, got = handle.blank_in_stream_push(None, finish=True, download=True)
                assert n_first == first_free and n_first + n_out == n_end
                parts.append(got)
            info = handle.blank_in_stream_info()
            assert torch.cuda.mem_get_info(DEV)[0] == free0, name
            assert info["n_pushed"] == len(x) and info["n_released"] == n_origin + len(x)
            got = np.concatenate(parts)
            assert got.tobytes() == y.tobytes(), (name, np.flatnonzero((got != y).reshape(len(x), -1).any(axis=1))[:8])
            assert np.array_equal(info["stats"], stats), (name, info["stats"], stats)
            # after finish only info and close are accepted
            with pytest.raises(_lib.Ft8rxError, match="finished"):
                handle.blank_in_stream_push(x[:1])
        finally:
            handle.blank_in_stream_close()


def test_stream_pushes_from_device_memory_and_leaves_other_streams_alone(handle):
    """on_device pushes of a sample-aligned chunk, with a down-converter stream opened and closed in between"""
    kind, B = bi.WIDE_IQ_I8, 256
    x, (y, stats, _), _, _ = cases.case(kind, B)
    d = _to_device(np.concatenate([np.zeros((1, 2), np.int8), x]))
    handle.blank_in_stream_open(kind, B, max_push=1000)
    try:
        parts, at = [], 0
        while at < len(x):
            n = min(1000, len(x) - at)
            parts.append(handle.blank_in_stream_push(None, d_ptr=d.data_ptr() + 2 * (1 + at), n=n, finish=at + n == len(x), download=True)[3])
            at += n
            if at == 2000:
                handle.ddc_wide_stream_open(dw.IQ_I8, 240000, [1000.0])
                handle.ddc_wide_stream_push(np.zeros((5000, 2), np.int8))
                handle.ddc_wide_stream_close()
        assert np.concatenate(parts).tobytes() == y.tobytes() and np.array_equal(handle.blank_in_stream_info()["stats"], stats)
    finally:
        handle.blank_in_stream_close()


def _noisy_stream(kind, rate, n, seed, impulses=200.0, peak=60.0):
    """Gaussian noise of `kind` with a carrier, plus impulses: something for the blanker to do and for the front end to filter"""
    rng = np.random.default_rng(seed)
    dt = bi._DTYPE[kind]
    sigma = {np.int16: 300.0, np.int8: 8.0, np.uint8: 8.0}[dt]
    t = np.arange(n) / rate
    tone = 3.0 * sigma * np.exp(2j * np.pi * 0.11 * rate * t)
    if bi.is_iq(kind):
        v = np.stack([tone.real, tone.imag], axis=1) + sigma * rng.standard_normal((n, 2))
    else:
        v = tone.real + sigma * rng.standard_normal(n)
    info = np.iinfo(dt)
    x = np.clip(np.rint(v + (127.5 if dt == np.uint8 else 0.0)), info.min, info.max).astype(dt)
    return bi.add_impulses(x, kind, rng, impulses, rate, peak)


@pytest.mark.parametrize("kind,rate,name", [(bi.WIDE_IQ_U8, 240000, "ddc_wide"), (bi.WIDE_IQ_I16, 240000, "ddc_wide"), (bi.REAL_I16, 44100, "ddc_rat")],
                         ids=["240k_iq_u8", "240k_iq_i16", "44k1_real_i16"])
def test_chain_into_the_front_end_on_the_device(handle, kind, rate, name):
    """Blanker stream -> the front end's stream push on the device, about 0.25 s: ddc_stream_read gives, byte for byte, what the same
    front-end stream gives when it is fed from the host with the twin's blanked samples"""
    n, B = rate // 4, 256
    x = _noisy_stream(kind, rate, n, 77)
    y, stats, _ = bi.reference(x, kind, B)
    assert stats[0] >= 20
    dial = [0.11 * rate - 1500.0] if bi.is_iq(kind) else [0.11 * rate - 1500.0]
    push = getattr(handle, name + "_stream_push")
    chunks = _cut(x, [7000] * (n // 7000) + ([n % 7000] if n % 7000 else []))
    # the chain on the device
    getattr(handle, name + "_stream_open")(kind, rate, dial)
    handle.blank_in_stream_open(kind, B, max_push=7000)
    released, m = [], 0
    try:
        for i, ch in enumerate(chunks):
            d_out, n_first, n_out = handle.blank_in_stream_push(ch, finish=i == len(chunks) - 1)
            released.append(n_out)
            if n_out:
                m = push(None, d_ptr=d_out, n=n_out)
        assert sum(released) == n and m > 0
        got = handle.ddc_stream_read(0, m)
        got_stats = handle.blank_in_stream_info()["stats"]
    finally:
        handle.blank_in_stream_close()
        getattr(handle, name + "_stream_close")()
    # the same front-end stream from the host, in the same pushes
    getattr(handle, name + "_stream_open")(kind, rate, dial)
    try:
        for part in _cut(y, released):
            if len(part):
                m2 = push(part)
        want = handle.ddc_stream_read(0, m2)
    finally:
        getattr(handle, name + "_stream_close")()
    assert m2 == m and np.array_equal(got_stats, stats)
    assert got.tobytes() == want.tobytes() and np.abs(want).max() > 0


def test_refusals_name_the_argument(handle):
    L, h = handle._L, handle._h
    host = np.zeros(4096, np.int16)
    d = _to_device(host)
    p = d.data_ptr()

    def err():
        return L.ft8rx_last_error(h).decode()
    ok = (bi.WIDE_IQ_U8, 1000, 1024, 1408, 6, 6)
    for i, v, name in ((0, 1, "kind"), (0, 3, "kind"), (0, 20, "kind"), (1, 0, "n_samples"), (2, 255, "block"), (2, 768, "block"), (2, 8192, "block"),
                       (3, 511, "threshold_q8"), (3, 16385, "threshold_q8"), (4, 65, "guard"), (4, -1, "guard"), (5, 65, "taper"), (5, -1, "taper")):
        args = list(ok)
        args[i] = v
        assert L.ft8rx_blank_in(h, p, *args, None, None, None) == -1 and name in err(), (name, err())
        assert L.ft8rx_blank_in_host(h, host.ctypes.data, *args, None, None) == -1 and name in err()
        if i != 1:
            assert L.ft8rx_blank_in_stream_open(h, args[0], *args[2:], 0, 1000) == -1 and name in err()
    assert L.ft8rx_blank_in(h, None, *ok, None, None, None) == -1 and "d_samples" in err()
    assert L.ft8rx_blank_in(h, p + 1, bi.WIDE_REAL_I16, 100, 256, 2048, 6, 6, None, None, None) == -1 and "d_samples" in err()
    assert L.ft8rx_blank_in_host(h, None, *ok, None, None) == -1 and "samples" in err()
    # the stream: a push, info or close without an open, a second open, n_new beyond max_push, max_push itself
    assert L.ft8rx_blank_in_stream_push(h, p, 10, 1, 0, None, None, None) == -1 and "no input blanker stream is open" in err()
    assert L.ft8rx_blank_in_stream_info(h, None, None, None) == -1 and L.ft8rx_blank_in_stream_close(h) == -1
    assert L.ft8rx_blank_in_stream_open(h, bi.WIDE_IQ_U8, 256, 1408, 6, 6, 0, 0) == -1 and "max_push" in err()
    assert L.ft8rx_blank_in_stream_open(h, bi.WIDE_IQ_U8, 256, 1408, 6, 6, 0, 1000) == 0
    try:
        assert L.ft8rx_blank_in_stream_open(h, bi.WIDE_IQ_U8, 256, 1408, 6, 6, 0, 1000) == -1 and "open on this handle already" in err()
        assert L.ft8rx_blank_in_stream_push(h, p, 1001, 1, 0, None, None, None) == -1 and "n_new" in err()
        assert L.ft8rx_blank_in_stream_push(h, None, 10, 0, 0, None, None, None) == -1 and "in is NULL" in err()
        assert L.ft8rx_blank_in_stream_push(h, p, 1000, 1, 0, None, None, None) == 0 and L.ft8rx_blank_in_stream_push(h, None, 0, 0, 0, None, None, None) == 0
    finally:
        assert L.ft8rx_blank_in_stream_close(h) == 0
    # the limits themselves are taken
    assert L.ft8rx_blank_in(h, p, bi.WIDE_REAL_I16, 4096, 4096, 512, 0, 0, None, None, None) == 0
    assert L.ft8rx_blank_in(h, p, bi.WIDE_IQ_I16, 2048, 256, 16384, 64, 64, None, None, None) == 0
    handle.sync()


# ---- Receiver
def _fields(d):
    return (" ".join(d["msg_tuple"]), d["their_snr"], d["fHz"], d["tsec"], d["decode_notes"])


@pytest.fixture(scope="module")
def cycle():
    """(240 kHz IQ int16 cycle with impulses, its dial, the twin's blanked samples and stats at the receiver's defaults)"""
    _, noisy, f_off, _, _ = cases.benefit_recipe()[0]
    noisy = np.concatenate([noisy, noisy[:3600000 - len(noisy)]])          # a whole cycle: 15 s
    y, stats, _ = bi.reference(noisy, bi.WIDE_IQ_I16, 256)
    return noisy, f_off, y, stats


def test_decode_stream_with_input_blanker_is_decode_stream_on_the_twin(cycle):
    noisy, f_off, y, stats = cycle
    rx = Receiver("", None, max_frames=1)
    try:
        assert rx.input_blanker is None and rx.input_blanker_stats is None
        want = rx.decode_stream(y, 240000, iq=True, dial_offsets_hz=[f_off])
        frame = rx._h.download_audio(rx._h.staging_ptr(), 1)
        got = rx.decode_stream(noisy, 240000, iq=True, dial_offsets_hz=[f_off], input_blanker=True)
        assert rx._h.download_audio(rx._h.staging_ptr(), 1).tobytes() == frame.tobytes()
        assert np.array_equal(rx.input_blanker_stats, stats) and stats[0] > 500
        assert [[_fields(d) for d in ch] for ch in got] == [[_fields(d) for d in ch] for ch in want] and len(want[0]) >= 10
        # a dict, and together with noise_blanker: the 12 kHz blanker works on the frame the input blanker left
        also = rx.decode_stream(noisy, 240000, iq=True, dial_offsets_hz=[f_off], input_blanker={"threshold": 5.5, "block": 256, "guard": 6, "taper": 6})
        assert [[_fields(d) for d in ch] for ch in also] == [[_fields(d) for d in ch] for ch in want]
        # refusals through the keyword: two streams, a float kind, a bad block
        two = np.zeros((2, 48000, 2), np.int16)
        with pytest.raises(_lib.Ft8rxError, match="input_blanker.*2 streams"):
            rx.decode_stream(two, 48000, iq=True, dial_offsets_hz=[0.0, 0.0], input_blanker=True)
        with pytest.raises(_lib.Ft8rxError, match="input_blanker.*float"):
            rx.decode_stream(np.zeros(48000, np.float32), 48000, input_blanker=True)
        with pytest.raises(_lib.Ft8rxError, match="block"):
            rx.decode_stream(noisy, 240000, iq=True, dial_offsets_hz=[f_off], input_blanker={"block": 300})
    finally:
        rx.close()
    with pytest.raises(_lib.Ft8rxError, match="block"):
        Receiver("", None, max_frames=1, input_blanker={"block": 1000})
    both = Receiver("", None, max_frames=1, input_blanker=True, noise_blanker=True)
    try:
        got = both.decode_stream(noisy, 240000, iq=True, dial_offsets_hz=[f_off])
        assert np.array_equal(both.input_blanker_stats, stats)
        assert np.array_equal(both.blanker_stats, blanker.reference(frame)[1])
        assert len(got[0]) >= 10
    finally:
        both.close()


def _live(samples, f_off, **kw):
    """One live cycle through WideIn under a virtual clock, pushed in uneven chunks with a poll() after each, early pass included,
    waterfall on -> (messages, the input blanker's stats, the channel's search grid)"""
    rate, t_first = 240000, 15.0 * 1000
    vt, got = [t_first], []
    rx = Receiver("x", got.append, time_source=lambda: vt[0], sample_rate=rate, iq=True, dial_offsets_hz=[f_off], t_first=t_first,
                  early_decode_hop=320, waterfall=True, **kw)
    try:
        at, k, returned = 0, 0, []
        while at < len(samples):
            n = (24000, 50001, 7, 240000, 3000)[k % 5]
            vt[0] = t_first + min(at + n, len(samples)) / rate
            rx.wide_in.push(samples[at:at + n])
            returned += rx.poll()
            at, k = at + n, k + 1
        rx.wide_in.flush()
        returned += rx.poll()
        stats = rx.input_blanker_stats
        grid = rx.wide_in.search_grid[0].copy()
    finally:
        rx.stop()
    assert rx.thread_error is None and returned == got
    return [_fields(d) + (d["early"],) for d in got], stats, grid


def test_live_cycle_through_wide_in_is_the_twin_path(cycle):
    noisy, f_off, y, stats = cycle
    want, none, grid_want = _live(y, f_off)
    got, got_stats, grid = _live(noisy, f_off, input_blanker=True)
    assert none is None and np.array_equal(got_stats, stats)
    assert got == want and len(want) >= 10 and any(m[-1] for m in want)
    assert np.array_equal(grid, grid_want)                 # the waterfall shows the blanked input
