"""The spectrogram stage behind the streaming down-converter on the GPU (ft8rx_ddc_stream_grid_*, k_grid_stream).
Every comparison is np.array_equal on float32 rows against ft8rx_spectrogram -- the existing, oracle-pinned k_spectrogram -- run on a
SECOND handle over host frames assembled from ft8rx_ddc_stream_read (zeros before the origin and beyond the outputs produced): row q of
the grid opened at hop phase p0 is hop h of the frame cut at m_first = p0 + 480 (q - h).  No tolerance anywhere.

test_one_cycle_every_hop pushes 17 one-second chunks, one more than the 16 s that would do for rows 1 .. 375: row 400 ends at output
192000, and 16 s of input produce 191520 outputs (whole tiles, a filter's reach behind)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import ddc_cases as cases
from pyft8_amd import _lib, ddc, ddc_rat, ddc_wide, synth
from pyft8_amd.receiver import Receiver

pytestmark = pytest.mark.gpu

NSAMP, HOP, TILE, WIN = 180000, 480, 1008, 3840
RATE, D = 24000, 2                          # 24 kHz IQ int16: D = 2, the cheapest
SRC = [1, 0, 1]                             # 3 channels out of 2 streams
DIALS = [-0.5 * RATE + 400.5, 0.11 * RATE + 33.3, 0.5 * RATE - 700.25]

_data = {}


def iq(n, key):
    """Two streams of full-scale random IQ int16 [2, n, 2]"""
    if (n, key) not in _data:
        rng = np.random.Generator(np.random.Philox(key=0x6A1D + key))
        x = rng.integers(-32768, 32768, size=(2, n, 2), dtype=np.int64).astype(np.int16)
        x.setflags(write=False)
        _data[(n, key)] = x
    return _data[(n, key)]


@pytest.fixture(scope="module", params=[False, True], ids=["976", "wide-1920"])
def layouts(request):
    """(stream handle, reference handle) of libft8rx.so, and of libft8rx_wide.so (1920 columns) for the tests that ask for both"""
    cfg = _lib.default_config(f0_hi=1500) if request.param else None
    h, ref = _lib.Handle(cfg, device=0, max_frames=3), _lib.Handle(cfg, device=0, max_frames=3)
    assert h.wide == request.param and h.grid_cols == (1920 if request.param else 976)
    yield h, ref
    h.close()
    ref.close()


@pytest.fixture(scope="module")
def handles():
    h, ref = _lib.Handle(device=0, max_frames=3), _lib.Handle(device=0, max_frames=3)
    yield h, ref
    h.close()
    ref.close()


def close(h):
    for name, field in (("ddc_wide_stream_close", "_wds"), ("ddc_rat_stream_close", "_rts")):
        if getattr(h, field) is not None:
            getattr(h, name)()
    if h._ds is not None:
        h.ddc_stream_close()


def frames_at(h, m_first, m_origin=0):
    """The frames [n_out][180000] of the outputs from m_first on, assembled on the host from ft8rx_ddc_stream_read: zeros before the
    origin and from m_produced on (the zero rule of ft8rx_ddc_stream_frame)"""
    m_done = h.ddc_stream_info()["m_produced"]
    f = np.zeros((h._ds[2], NSAMP), np.int16)
    lo, hi = max(m_first, m_origin), min(m_first + NSAMP, m_done)
    if hi > lo:
        f[:, lo - m_first:hi - m_first] = h.ddc_stream_read(lo, hi - lo)
    return f


def rows_equal_frame(h, ref, p0, q_lo, q_hi, hop_of_q_lo, m_origin=0, rows=None):
    """rows q_lo .. q_hi - 1 of every channel == hops hop_of_q_lo .. of the frame cut at p0 + 480 (q_lo - hop_of_q_lo)"""
    n = q_hi - q_lo
    assert n >= 1 and 1 <= hop_of_q_lo and hop_of_q_lo + n - 1 <= 375
    got = h.ddc_stream_grid_read(q_lo, n) if rows is None else rows
    want = ref.spectrogram(frames_at(h, p0 + HOP * (q_lo - hop_of_q_lo), m_origin))[:, hop_of_q_lo:hop_of_q_lo + n]
    assert got.shape == want.shape == (h._ds[2], n, h.grid_cols) and got.dtype == want.dtype == np.float32
    bad = [(j, q_lo + i) for j in range(got.shape[0]) for i in range(n) if not np.array_equal(got[j, i], want[j, i])]
    assert not bad, f"{len(bad)} of {got.shape[0] * n} rows differ, first (channel, q) {bad[:5]}"
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))                    # the bytes
    return got


def push_all(h, x, lens, between=None):
    at, i = 0, 0
    while at < x.shape[1]:
        n = min(lens[i % len(lens)], x.shape[1] - at)
        m = h.ddc_stream_push(x[:, at:at + n])
        at, i = at + n, i + 1
        if between is not None and at >= x.shape[1] // 2 > at - n:
            between()
    return m


# ---- 1. one cycle, every hop
def test_one_cycle_every_hop(handles):
    h, ref = handles
    x = iq(17 * RATE, 1)
    try:
        h.ddc_stream_open(ddc.IQ_I16, RATE, 2, SRC, DIALS)
        h.ddc_stream_grid_open(0, 750)
        assert h.ddc_stream_grid_info() == {"q_first_held": 1, "q_next": 1, "cols": 976, "n_rows": 750}
        m = push_all(h, x, [RATE])
        info = h.ddc_stream_grid_info()
        assert m >= 400 * HOP and info["q_first_held"] == 1 and info["q_next"] == m // HOP + 1 >= 401
        g = rows_equal_frame(h, ref, 0, 1, 376, 1)                                  # rows 1 .. 375 = hops 1 .. 375 of the frame at the origin
        assert g.max() > 60.0 and g.min() > -100.0                                  # a real signal: full-scale noise, no empty bins
        rows_equal_frame(h, ref, 0, 383, 401, 8)                                    # rows 383 .. 400 = hops 8 .. 25 of the frame cut at 480 x 375
    finally:
        close(h)


# ---- 2. odd and extreme phase, 8. both layouts
def phase_case(h, ref, p0):
    x = iq(2 * RATE, 2)
    try:
        h.ddc_stream_open(ddc.IQ_I16, RATE, 2, SRC, DIALS)
        h.ddc_stream_grid_open(p0, 750)
        m = push_all(h, x, [RATE])
        info = h.ddc_stream_grid_info()
        q_next = (m - p0) // HOP + 1
        assert info["q_first_held"] == 0 and info["q_next"] == q_next > 40 and info["cols"] == h.grid_cols
        rows_equal_frame(h, ref, p0, 0, q_next, 8)                                  # every row, h = q + 8: m_first = p0 - 3840, before the origin
        rows_equal_frame(h, ref, p0, 0, 7, 1)                                       # the first seven rows as hops 1 .. 7: m_first = p0 - 480
        rows_equal_frame(h, ref, p0, 12, q_next, 9)                                 # ... and a frame that begins inside the stream: m_first = p0 + 1440
    finally:
        close(h)


@pytest.mark.parametrize("p0", [1, 137, 479])
def test_odd_and_extreme_phase(handles, p0):
    phase_case(*handles, p0)


def test_both_layouts(layouts):
    phase_case(*layouts, 137)


# ---- 3. the output ring's wrap
@pytest.mark.parametrize("p0", [0, 137])
def test_output_ring_wrap(handles, p0):
    """The first output index is 1008 x 357 = 359856: m passes 360000 inside the first window, and every later window of the two
    seconds lies across or behind the wrap"""
    h, ref = handles
    m0 = TILE * 357
    x = iq(2 * RATE, 3)
    try:
        h.ddc_stream_open(ddc.IQ_I16, RATE, 2, SRC, DIALS, n_origin=m0 * D)
        h.ddc_stream_grid_open(p0, 750)
        m = push_all(h, x, [RATE])
        info = h.ddc_stream_grid_info()
        q0 = (m0 - p0) // HOP + 1
        assert q0 == 750 and p0 + HOP * q0 > m0 >= p0 + HOP * (q0 - 1)
        assert info["q_first_held"] == q0 and info["q_next"] == (m - p0) // HOP + 1 > q0 + 40 and m > 360000 + 2 * WIN
        rows_equal_frame(h, ref, p0, q0, info["q_next"], 8, m_origin=m0)
        rows_equal_frame(h, ref, p0, q0, q0 + 7, 1, m_origin=m0)
    finally:
        close(h)


# ---- 4. the grid ring's wrap, and the refusals
def test_grid_ring_wrap_and_refusals(handles):
    h, ref = handles
    L, hp = h._L, h._h
    err = lambda: L.ft8rx_last_error(hp).decode()                                       # noqa: E731
    x = iq(RATE + RATE // 5, 4)                                                         # 1.2 s
    buf = np.zeros((3, 16, 976), np.float32)
    try:
        assert L.ft8rx_ddc_stream_grid_open(hp, 0, 16) == -1 and "no stream is open" in err()
        assert L.ft8rx_ddc_stream_grid_info(hp, None, None, None, None) == -1 and "no grid is open" in err()
        assert L.ft8rx_ddc_stream_grid_read(hp, 1, 1, buf.ctypes.data) == -1 and "no grid is open" in err()
        h.ddc_stream_open(ddc.IQ_I16, RATE, 2, SRC, DIALS)
        assert L.ft8rx_ddc_stream_grid_info(hp, None, None, None, None) == -1 and "no grid is open" in err()
        for p0 in (-1, 480):
            assert L.ft8rx_ddc_stream_grid_open(hp, p0, 16) == -1 and f"hop_phase {p0} outside [0, 480)" in err()
        for n_rows in (15, 751, 0, -3):
            assert L.ft8rx_ddc_stream_grid_open(hp, 0, n_rows) == -1 and f"n_rows {n_rows} outside [16, 750]" in err()
        h.ddc_stream_grid_open(5, 16)
        assert L.ft8rx_ddc_stream_grid_open(hp, 5, 16) == -1 and "open already" in err()
        assert h.ddc_stream_grid_info() == {"q_first_held": 0, "q_next": 0, "cols": 976, "n_rows": 16}
        assert L.ft8rx_ddc_stream_grid_read(hp, 0, 1, buf.ctypes.data) == -1 and "it holds 0 .. 0" in err()
        m = push_all(h, x, [4001, 333, 7000])
        q_next = (m - 5) // HOP + 1
        info = h.ddc_stream_grid_info()
        assert q_next >= 16 + 12 and info =={"q_first_held": q_next - 16, "q_next": q_next, "cols": 976, "n_rows": 16}
        held = f"it holds {q_next - 16} .. {q_next}"
        assert L.ft8rx_ddc_stream_grid_read(hp, q_next - 17, 1, buf.ctypes.data) == -1 and held in err() and f"rows [{q_next - 17}, {q_next - 16})" in err()
        assert L.ft8rx_ddc_stream_grid_read(hp, 0, 1, buf.ctypes.data) == -1 and held in err()
        assert L.ft8rx_ddc_stream_grid_read(hp, q_next, 1, buf.ctypes.data) == -1 and held in err()           # not yet produced
        assert L.ft8rx_ddc_stream_grid_read(hp, q_next - 3, 4, buf.ctypes.data) == -1 and held in err()
        assert L.ft8rx_ddc_stream_grid_read(hp, q_next - 16, 0, buf.ctypes.data) == -1 and held in err()
        assert L.ft8rx_ddc_stream_grid_read(hp, q_next - 16, 16, None) == -1 and "rows is NULL" in err()
        rows_equal_frame(h, ref, 5, q_next - 16, q_next, 8)                             # the 16 held rows, after the wrap
        assert not buf.any()                                                            # a refused read writes nothing
        h.ddc_stream_close()
        assert L.ft8rx_ddc_stream_grid_info(hp, None, None, None, None) == -1           # released with the stream
        # after a push the grid can no longer be opened
        h.ddc_stream_open(ddc.IQ_I16, RATE, 2, SRC, DIALS)
        h.ddc_stream_push(x[:, :1])
        assert L.ft8rx_ddc_stream_grid_open(hp, 0, 16) == -1 and "before the first push" in err()
    finally:
        close(h)


# ---- 5. chunk invariance
def test_chunk_invariance(handles):
    h, ref = handles
    x = iq(2 * RATE, 5)
    got = []
    try:
        for lens in ([RATE], [1, 479 * D, 7 * D + 3]):
            h.ddc_stream_open(ddc.IQ_I16, RATE, 2, SRC, DIALS)
            h.ddc_stream_grid_open(137, 750)
            m = push_all(h, x, lens, between=(lambda: h.ddc(iq(5000 * D, 6), ddc.IQ_I16, RATE, SRC, DIALS)) if len(lens) > 1 else None)
            info = h.ddc_stream_grid_info()
            got.append((m, info, h.ddc_stream_grid_read(info["q_first_held"], info["q_next"] - info["q_first_held"])))
            if len(lens) > 1:
                rows_equal_frame(h, ref, 137, 0, info["q_next"], 8, rows=got[-1][2])
            h.ddc_stream_close()
    finally:
        close(h)
    assert got[0][0] == got[1][0] and got[0][1] == got[1][1] and got[0][1]["q_next"] > 40
    assert got[0][2].tobytes() == got[1][2].tobytes()


# ---- 6. silence
def test_silence(handles):
    h, _ = handles
    try:
        h.ddc_stream_open(ddc.IQ_I16, RATE, 2, SRC, DIALS)
        h.ddc_stream_grid_open(3, 750)
        h.ddc_stream_push(np.zeros((2, RATE, 2), np.int16))
        info = h.ddc_stream_grid_info()
        g = h.ddc_stream_grid_read(0, info["q_next"])
        assert info["q_next"] > 20 and g.shape == (3, info["q_next"], 976) and (g == np.float32(-240.0)).all()
    finally:
        close(h)


# ---- 7. the other two front ends
@pytest.mark.parametrize("front", ["wide", "rat"])
def test_other_front_ends(handles, front):
    """A 240 kHz IQ uint8 stream through ft8rx_ddc_wide_stream_*, a 44 100 Hz real int16 stream through ft8rx_ddc_rat_stream_*: the
    same grid calls, the rows are the spectrogram of the frames read from the same ring"""
    h, ref = handles
    rng = np.random.Generator(np.random.Philox(key=0x6A1D + 70))
    try:
        if front == "wide":
            rate = 240000
            x = rng.integers(0, 256, size=(rate + rate // 2, 2), dtype=np.int64).astype(np.uint8)
            h.ddc_wide_stream_open(ddc_wide.IQ_U8, rate, [-50000.5, 70000.25])
            push = h.ddc_wide_stream_push
        else:
            rate = 44100
            x = rng.integers(-32768, 32768, size=rate + rate // 2, dtype=np.int64).astype(np.int16)
            h.ddc_rat_stream_open(ddc_rat.REAL_I16, rate, [1000.0, 9000.25])
            push = h.ddc_rat_stream_push
        h.ddc_stream_grid_open(137, 750)
        with pytest.raises(_lib.Ft8rxError, match="open already"):
            h.ddc_stream_grid_open(137, 750)
        cuts = [0, 7, rate // 3, rate, len(x)]
        for lo, hi in zip(cuts, cuts[1:]):
            m = push(x[lo:hi])
        info = h.ddc_stream_grid_info()
        assert m > 12000 and info["q_first_held"] == 0 and info["q_next"] == (m - 137) // HOP + 1
        g = rows_equal_frame(h, ref, 137, 0, info["q_next"], 8)
        assert g.max() > 20.0
        # a fresh stream of the same kind: after its first push the grid can no longer be opened, and nothing of a grid exists
        close(h)
        if front == "wide":
            h.ddc_wide_stream_open(ddc_wide.IQ_U8, rate, [-50000.5, 70000.25])
            h.ddc_wide_stream_push(x[:7])
        else:
            h.ddc_rat_stream_open(ddc_rat.REAL_I16, rate, [1000.0, 9000.25])
            h.ddc_rat_stream_push(x[:7])
        with pytest.raises(_lib.Ft8rxError, match="before the first push"):
            h.ddc_stream_grid_open(1, 16)
        with pytest.raises(_lib.Ft8rxError, match="no grid is open"):
            h.ddc_stream_grid_info()
    finally:
        close(h)


# ---- 9. the live layer
def test_live_waterfall_and_search():
    """Receiver(sample_rate=24000, iq=True, two dials, waterfall=True) on a virtual clock whose first sample lies 343 outputs after a
    cycle start (m_c = -343, p0 = 137), fed 17 s: a synthetic frame of six signals at -8 .. +2 dB mixed up to the first dial, faint
    noise everywhere.  After the cycle: the channel grids against ft8rx_spectrogram of the frames the complete pass decoded, the
    waterfall views, search(channel=) against a 12 kHz Receiver that was given the same frame, and a candidate's ladder."""
    rate, t_first = RATE, 15000.0 + 343 / 12000
    audio = synth.make_frame(4242, n_signals=6, snr_range=(-8.0, 2.0))
    n = NSAMP * D
    spec = np.zeros(n, np.complex128)
    offs = cases.offsets(rate)
    cases._place(spec, audio, offs[0])
    rng = np.random.Generator(np.random.Philox(key=0x6A1D + 90))
    cyc = np.fft.ifft(spec) * n / NSAMP
    x = np.take(cyc, (np.arange(17 * rate) + 343 * D) % n)                              # sample 0 of the stream is output 343 of the cycle
    x = np.stack([x.real, x.imag], axis=1) + rng.normal(0.0, 3.0, size=(len(x), 2))
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    vt, got = [t_first], []
    rx = Receiver("x", got.append, time_source=lambda: vt[0], sample_rate=rate, iq=True, dial_offsets_hz=offs, bands=("20m", "17m"),
                  t_first=t_first, waterfall=True, autostart=False)
    ctl = Receiver("", None)
    try:
        w = rx.wide_in
        for at in range(0, len(x), rate):
            w.push(x[at:at + rate])
            vt[0] = t_first + (at + rate) / rate
        assert w.grid_phase == 137 and w.sched.cycle_start(1000) == -343 and w.m_produced >= NSAMP - 343 + 40 * HOP
        msgs = rx.poll()
        assert any(d["channel"] == 0 for d in msgs) and not any(d["channel"] == 1 for d in msgs)
        # the frames the complete pass decoded: outputs [-343, 179657) of each channel
        with rx._live_lock:
            live = rx._live
            frames = np.zeros((2, NSAMP), np.int16)
            frames[:, 343:] = live.ddc_stream_read(0, NSAMP - 343)
            live.ddc_stream_frame(-343, NSAMP)
            assert np.array_equal(live.download_audio(live.staging_ptr(), 2), frames)
        assert w.grid_cycle(0) == 1000 and w.grid_cycle(1) is None
        width = ctl.audio_in.search_grid.shape[1]
        want = ctl._handle(1).spectrogram(frames[0])[0], ctl._handle(1).spectrogram(frames[1])[0]
        for j in range(2):
            assert w.search_grid[j].shape == (750, width) and w.search_grid[j].dtype == np.float32
            assert np.array_equal(w.search_grid[j][8:376], want[j][8:376, :width])
            assert np.array_equal(w.search_grid[j][1:8], want[j][1:8, :width])         # (only zeros lie before this frame)
            assert (w.search_grid[j][376 + 60:] == 1.0).all() and (w.search_grid[j][0] == 1.0).all()      # the odd half: barely begun
            assert not np.array_equal(w.search_grid[j][377], np.ones(width, np.float32))
            wf = w.waterfall_data[j]
            assert np.shares_memory(wf["data"], w.search_grid[j]) and np.array_equal(wf["data"], w.search_grid[j][::2, ::2].T)
            assert {k: v for k, v in wf.items() if k != "data"} == {k: v for k, v in ctl.audio_in.waterfall_data.items() if k != "data"}
        n_compared = []
        for j in range(2):
            ctl.audio_in.load_frame(frames[j])
            a = [(c.origin["f0_idx"], c.origin["h0_idx"], c.origin["score"]) for c in rx.search("150000_000000", 0, channel=j)]
            cands = list(rx.candidates)
            b = [(c.origin["f0_idx"], c.origin["h0_idx"], c.origin["score"]) for c in ctl.search("150000_000000", 0)]
            assert [c for c in a if c[1] >= 2] == [c for c in b if c[1] >= 2] and a == b
            n_compared.append(len([c for c in a if c[1] >= 2]))
            assert all(c.origin["channel"] == j and c.origin["band"] == ("20m", "17m")[j] for c in cands)
            assert all("channel" not in c.origin for c in ctl.candidates)
            if j == 0:                                                                  # the best candidate's ladder, as on the 12 kHz path
                ca, cb = cands[0], ctl.candidates[0]
                for step in range(6):
                    ca.on_message = cb.on_message = None
                    ca.decode(step)
                    cb.decode(step)
                assert ca.decode_result == cb.decode_result and ca.tweaks == cb.tweaks and ca.decode_notes == cb.decode_notes
                assert ca.decode_result not in (None, "stop")
        print(f"candidates compared (h0 >= 2): channel 0 {n_compared[0]}, channel 1 {n_compared[1]}")
        assert n_compared[0] >= 6                                                       # the six signals at the least
        with pytest.raises(_lib.Ft8rxError, match=r"channels 0 \.\. 1"):
            rx.search("150000_000000", 0, channel=2)
        with pytest.raises(_lib.Ft8rxError, match="waterfall=True"):
            ctl.search("150000_000000", 0, channel=0)
    finally:
        rx.close()
        ctl.close()


def test_off_allocates_and_launches_nothing(handles):
    """Without grid_open a stream holds no grid: info and read refuse, and the pushes leave the device memory in use where it was"""
    h, _ = handles
    L, hp = h._L, h._h
    try:
        h.ddc_stream_open(ddc.IQ_I16, RATE, 2, SRC, DIALS)
        free0 = torch.cuda.mem_get_info(0)[0]
        h.ddc_stream_push(iq(RATE, 7))
        h.sync()
        assert torch.cuda.mem_get_info(0)[0] == free0
        assert L.ft8rx_ddc_stream_grid_info(hp, None, None, None, None) == -1 and "no grid is open" in L.ft8rx_last_error(hp).decode()
        q = C.c_uint64()
        assert L.ft8rx_ddc_stream_grid_info(hp, C.byref(q), None, None, None) == -1
    finally:
        close(h)
