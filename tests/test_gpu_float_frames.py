"""Float32 frames on the GPU: the _f32 entries against their int16 twins on integer-valued input (byte for
byte), under power-of-two scaling (the grid shifts, the messages stay), on streams so quiet that their int16 frames are zero, out of
the streaming down-converter's float32 ring (frames, waterfall rows), through the subtraction and through the live receiver."""
import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import float_frames_cases as F
from pyft8_amd import _lib, ddc, ddc_wide
from pyft8_amd.receiver import Receiver

pytestmark = pytest.mark.gpu

NSAMP = 180000
TILE = 1008


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle(device=0, max_frames=16)
    yield h
    h.close()


@pytest.fixture(scope="module")
def int_path(handle):
    """The int16 entries on the four frames, computed once: grid, cycle spectrum, batch results, message texts"""
    a = F.int_frames()
    res = handle.decode_batch(a)
    msgs, mcnt = _lib.package_batch(*res)
    return {"grid": handle.spectrogram(a), "spec": handle.cycle_spectrum(a), "res": res, "texts": texts_of(msgs, mcnt)}


def texts_of(msgs, mcnt):
    from pyft8_amd import messages as M
    return [[" ".join(d["msg_tuple"]) for d in M.message_dicts(msgs[f], mcnt[f], cyclestart_string="700101_000015", band=None, odd_even=0)]
            for f in range(len(mcnt))]


def same_results(got, want, what):
    """records the counts cover, counts, events as a set (the log is written in arrival order), event counts"""
    assert got[1].tobytes() == want[1].tobytes() and got[3].tobytes() == want[3].tobytes(), what
    for f in range(len(want[1])):
        nc, ne = int(want[1][f]), min(int(want[3][f]), _lib.EVENT_CAP)
        assert got[0][f, :nc].tobytes() == want[0][f, :nc].tobytes(), (what, f)
        assert sorted(e.tobytes() for e in got[2][f, :ne]) == sorted(e.tobytes() for e in want[2][f, :ne]), (what, f)


# ---- 1. integer-valued floats are the int16 path, byte for byte
def test_stage_entries_equal_the_int16_entries(handle, int_path):
    af = F.int_frames().astype(np.float32)
    assert handle.spectrogram_f32(af).tobytes() == int_path["grid"].tobytes()
    assert handle.cycle_spectrum_f32(af).tobytes() == int_path["spec"].tobytes()
    assert int_path["grid"][:2, 1:].min() > -200 and int_path["grid"][2, 1:].max() == -240.0      # real frames; the zero frame is the floor


def test_batch_equals_the_int16_batch_single_chain(handle, int_path):
    af = F.int_frames().astype(np.float32)
    want = int_path["res"]
    assert want[1][:2].min() > 0 and sum(len(t) for t in int_path["texts"]) > 10
    same_results(handle.decode_batch_f32(af), want, "decode_batch_f32")
    handle.enqueue_f32(handle.staging_ptr_f32(), 4)                                 # the synchronous entry left the frames in the float staging
    same_results(handle.fetch(4), want, "enqueue_batch_f32")
    pinned = handle.pinned_bytes(af.nbytes).view(np.float32).reshape(af.shape)
    pinned[:] = af
    for _ in range(3):                                                              # both float staging buffers
        handle.enqueue_host_f32(pinned)
        same_results(handle.fetch(4), want, "enqueue_batch_host_f32")
    m, c = handle.decode_messages_f32(af)
    assert texts_of(m, c) == int_path["texts"]


@pytest.mark.parametrize("n_streams", [1, 2])
def test_batch_equals_the_int16_batch_in_chunks(handle, n_streams):
    """16 frames: the smallest batch that is cut into two chunks (batch_plan.hpp: at least 8 frames per chunk) -- the synchronous entry
    copies chunk by chunk (sized by the sample bytes), the device entry runs free-running chunk streams; with one stream, one chain"""
    a = np.concatenate([np.roll(F.int_frames(), k, axis=0) for k in range(4)])
    af = a.astype(np.float32)
    handle.set_streams(n_streams)
    try:
        want = handle.decode_batch(a)
        assert want[1].max() > 0
        same_results(handle.decode_batch_f32(af), want, "decode_batch_f32")
        for _ in range(2):
            handle.enqueue_f32(handle.staging_ptr_f32(), 16)
            same_results(handle.fetch(16), want, "enqueue_batch_f32")
        handle.enqueue_host_f32(af)
        same_results(handle.fetch(16), want, "enqueue_batch_host_f32")
    finally:
        handle.set_streams(2)


# ---- 2. scale
@pytest.mark.parametrize("log2", [-1, -20])
def test_scale_shifts_the_grid_and_keeps_the_messages(handle, int_path, log2):
    """Power-of-two scaling is exact through the window and the FFT; the contract's log10f bound of 3e-6 applies twice, times ten,
    plus one float ulp at 128 dB (7.6e-6): under 1e-4 dB, doubled"""
    af = F.int_frames().astype(np.float32) * np.float32(2.0 ** log2)
    shift = 20.0 * np.log10(2.0) * log2
    g = handle.spectrogram_f32(af)[:, 1:].astype(np.float64)
    gi = int_path["grid"][:, 1:].astype(np.float64)
    keep = (gi > -200.0) & (gi + shift > -239.9)                                     # not the floor of either path
    assert keep[:2].all() and keep.mean() > 0.6
    err = np.abs(g - (gi + shift))[keep].max()
    print(f"scale 2^{log2}: {keep.sum()} grid values, max |error| {err:.3e} dB")
    assert err <= 2e-4
    if log2 == -20:
        m, c = _lib.package_batch(*handle.decode_batch_f32(af))
        assert texts_of(m, c) == int_path["texts"]


# ---- 3. the case the feature exists for: a stream whose int16 frames are zero
@pytest.fixture(scope="module")
def rx():
    r = Receiver("", None, max_frames=2)
    yield r
    r.close()


@pytest.fixture(scope="module")
def full_level_texts(rx):
    res = rx.decode_stream(F.full_stream()[None], F.RATE, iq=True, dial_offsets_hz=F.offsets())
    t = [[" ".join(d["msg_tuple"]) for d in ch] for ch in res]
    assert min(len(x) for x in t) > 5
    return t


def test_quiet_stream_decodes_as_at_full_level(handle, rx, full_level_texts):
    q = F.quiet_stream()
    handle.ddc(q[None], ddc.IQ_F32, F.RATE, [0, 0], F.offsets())                    # through ft8rx_ddc_host: the int16 frames
    assert not handle.download_audio(handle.staging_ptr(), 2).any()                  # |y| < 0.5 everywhere
    assert [len(ch) for ch in rx.decode_stream(q[None], F.RATE, iq=True, dial_offsets_hz=F.offsets())] == [0, 0]
    got = rx.decode_stream(q[None], F.RATE, iq=True, dial_offsets_hz=F.offsets(), float_frames=True)
    assert [[" ".join(d["msg_tuple"]) for d in ch] for ch in got] == full_level_texts


def test_quiet_wide_stream_decodes_as_at_full_level(handle, rx):
    """240 kHz IQ int16 through the wide pre-decimator: the stream times 64 is the same information at a level the int16 path holds"""
    x = F.wide_quiet_stream()
    offs = list(F.wide_offsets())
    handle.ddc_wide(x, ddc_wide.kind_of(x, True), F.WIDE_RATE, offs)
    assert not handle.download_audio(handle.staging_ptr(), 2).any()
    assert [len(ch) for ch in rx.decode_stream(x, F.WIDE_RATE, iq=True, dial_offsets_hz=offs)] == [0, 0]
    want = rx.decode_stream(x * np.int16(F.WIDE_UP), F.WIDE_RATE, iq=True, dial_offsets_hz=offs)
    got = rx.decode_stream(x, F.WIDE_RATE, iq=True, dial_offsets_hz=offs, float_frames=True)
    t = [[" ".join(d["msg_tuple"]) for d in ch] for ch in got]
    assert t == [[" ".join(d["msg_tuple"]) for d in ch] for ch in want] and min(len(c) for c in t) >= 4


# ---- 4. stream: frames out of the float32 ring
def _iq(n, key):
    rng = np.random.Generator(np.random.Philox(key=0xF32 + key))
    return rng.integers(-32768, 32768, size=(2, n, 2), dtype=np.int64).astype(np.int16)


SRC, RATE24 = [1, 0, 1], 24000


def _dials(rate):
    return [-0.5 * rate + 400.5, 0.11 * rate + 33.3, 0.5 * rate - 700.25]


@pytest.fixture()
def stream(handle):
    def open_(keep_f32=True):
        return handle.ddc_stream_open(ddc.IQ_I16, RATE24, 2, SRC, _dials(RATE24), keep_f32=keep_f32)
    yield open_
    if handle._ds is not None:
        handle.ddc_stream_close()


def _frames_f32(handle, m_first, n_have, m):
    """the gathered float frames, checked against the ring's own bytes (ddc_stream_read's y_f32)"""
    handle.ddc_stream_frame_f32(m_first, n_have)
    got = handle.download_audio_f32(handle.staging_ptr_f32(), 3)
    want = np.zeros((3, NSAMP), np.float32)
    lo, hi = max(m_first, 0), min(m_first + n_have, m)
    if hi > lo:
        want[:, lo - m_first:hi - m_first] = handle.ddc_stream_read(lo, hi - lo, want_float=True)[1]
    assert got.tobytes() == want.tobytes(), (m_first, n_have)
    return got


def test_stream_frames_are_the_float_ring(handle, stream):
    x = _iq(3 * RATE24, 1)
    seen = []
    for lens in ([RATE24] * 3, [7000, 17000, 24000, 1, 23999]):
        stream()
        at = 0
        for n in lens:
            m = handle.ddc_stream_push(x[:, at:at + n])
            at += n
        assert 30000 < m < 36000
        a = _frames_f32(handle, 1001, NSAMP, m)                                      # odd; past m_produced: a zero tail
        assert a[:, :m - 1001].std() > 1000 and not a[:, m - 1001:].any()
        assert np.abs(a - np.rint(a)).max() > 0.1                                    # unrounded
        b = _frames_f32(handle, -6001, NSAMP, m)                                     # negative and odd: a zero head
        assert not b[:, :6001].any() and b[:, 6001:6001 + m].std() > 1000
        c = _frames_f32(handle, 2000, 5000, m)                                       # n_have < 180000
        assert c[:, :5000].std() > 1000 and not c[:, 5000:].any()
        seen.append((a.tobytes(), b.tobytes(), c.tobytes()))
        handle.ddc_stream_close()
    assert seen[0] == seen[1]                                                        # two chunkings of the pushes
    # the first cycle is the one-shot's float output
    xs = x[:, :5000 * 2]
    _, y1 = handle.ddc(xs, ddc.IQ_I16, RATE24, SRC, _dials(RATE24), want_float=True)
    stream()
    assert handle.ddc_stream_push(xs) == 4 * TILE
    handle.ddc_stream_frame_f32(0, 4 * TILE)
    assert handle.download_audio_f32(handle.staging_ptr_f32(), 3)[:, :4 * TILE].tobytes() == y1[:, :4 * TILE].tobytes()


def test_stream_frame_refusals(handle, stream):
    stream(keep_f32=False)
    x = _iq(RATE24, 2)
    m = handle.ddc_stream_push(x)
    with pytest.raises(_lib.Ft8rxError, match="keep_f32"):
        handle.ddc_stream_frame_f32(0, NSAMP)
    handle.ddc_stream_frame(0, NSAMP)                                                # the int16 entry serves it as before
    handle.ddc_stream_close()
    stream()
    for _ in range(32):
        m = handle.ddc_stream_push(x)
    assert m > 2 * NSAMP + 20000
    _frames_f32(handle, 2 * NSAMP - 9999, 30000, m)                                  # wraps the output ring
    with pytest.raises(_lib.Ft8rxError, match="left the ring"):
        handle.ddc_stream_frame_f32(m - 2 * NSAMP - 1, NSAMP)
    with pytest.raises(_lib.Ft8rxError, match="n_have"):
        handle.ddc_stream_frame_f32(m - 1000, NSAMP + 1)


# ---- 5. waterfall rows of a float stream
def test_grid_rows_come_from_the_float_ring(handle):
    p0, n_rows = 137, 64
    x = _iq(RATE24, 3)
    handle.ddc_stream_open(ddc.IQ_I16, RATE24, 2, SRC, _dials(RATE24), keep_f32=2)
    try:
        handle.ddc_stream_grid_open(p0, n_rows)
        m = handle.ddc_stream_push(x)
        info = handle.ddc_stream_grid_info()
        assert info["q_first_held"] <= 3 < info["q_next"]

        def check(q, h):
            row = handle.ddc_stream_grid_read(q, 1)[:, 0]
            handle.ddc_stream_frame_f32(p0 + 480 * (q - h), NSAMP)
            fr = handle.download_audio_f32(handle.staging_ptr_f32(), 3)
            assert row.tobytes() == handle.spectrogram_f32(fr)[:, h].tobytes(), (q, h)
            assert row.tobytes() != handle.spectrogram(np.clip(np.rint(fr), -32768, 32767).astype(np.int16))[:, h].tobytes()   # not the int16 ring's
        check(3, 8)                                                                  # a zero prefix: the window starts before the origin
        for _ in range(30):
            m = handle.ddc_stream_push(x)
        q = (2 * NSAMP - p0) // 480 + 2                                              # the window [.., p0 + 480 q) crosses the ring's end
        assert p0 + 480 * q - 3840 < 2 * NSAMP < p0 + 480 * q <= m
        info = handle.ddc_stream_grid_info()
        assert info["q_first_held"] <= q < info["q_next"]
        check(q, 100)
    finally:
        handle.ddc_stream_close()


# ---- 6. subtraction
def test_subtract_f32_is_the_float_residual_of_the_int16_entry(handle, int_path):
    a = F.int_frames()
    res = int_path["res"]
    msgs, mcnt = _lib.package_batch(*res)
    sigs = _lib.subtraction_list(msgs, mcnt, res[0], -10)
    assert sigs[1][:2].min() > 3
    for refine in (0, 2):
        handle.decode_batch(a)                                                       # the frames into the int16 staging ...
        want = handle.subtract(handle.staging_ptr(), 4, (sigs[0].copy(), sigs[1].copy()), return_float=True, refine=refine)
        handle.decode_batch_f32(a.astype(np.float32))                                # ... and into the float staging
        got = handle.subtract(handle.staging_ptr_f32(), 4, (sigs[0].copy(), sigs[1].copy()), return_float=True, refine=refine, float_frames=True)
        assert got.tobytes() == want.tobytes(), refine
        assert handle.download_audio_f32(handle.staging_ptr_f32(), 4).tobytes() == got.tobytes()      # written back without rounding
        assert np.abs(got - np.rint(got)).max() > 0.1 and np.abs(got[:2] - a[:2]).max() > 100


def test_two_passes_keep_the_first_pass(rx):
    a = F.int_frames()[:2]
    one = rx.decode_frames(a.astype(np.float32), float_frames=True)
    two = rx.decode_frames(a.astype(np.float32), passes=2, float_frames=True)
    two_i = rx.decode_frames(a, passes=2)
    for f in range(2):
        first = [d for d in two[f] if "_SUB" not in d["decode_notes"]]
        assert [" ".join(d["msg_tuple"]) for d in first] == [" ".join(d["msg_tuple"]) for d in one[f]] and len(one[f]) > 5
        print(f"frame {f}: second-pass messages, float frames {len(two[f]) - len(first)}, int16 frames "
              f"{sum('_SUB' in d['decode_notes'] for d in two_i[f])}")


# ---- 7. live
def test_live_receiver_on_the_quiet_stream(full_level_texts):
    q, offs = F.quiet_stream(), F.offsets()
    t_first = 15.0 * 1000

    def run(**kw):
        vt, got = [t_first], []
        r = Receiver("x", got.append, time_source=lambda: vt[0], sample_rate=F.RATE, iq=True, dial_offsets_hz=offs, t_first=t_first,
                     early_decode_hop=None, **kw)
        try:
            assert r._thread is None
            for at in range(0, len(q), 40000):
                vt[0] = t_first + (at + 40000) / F.RATE
                r.wide_in.push(q[at:at + 40000])
                r.poll()
            r.wide_in.flush()
            r.poll()
        finally:
            r.stop()
        return got

    got = run(float_frames=True)
    for j in range(2):
        assert [" ".join(d["msg_tuple"]) for d in got if d["channel"] == j] == full_level_texts[j], j
    assert run() == []


def test_receiver_refuses_the_noise_blanker_with_float_frames():
    with pytest.raises(_lib.Ft8rxError, match="float_frames.*noise_blanker"):
        Receiver("", None, noise_blanker=True, float_frames=True)
    r = Receiver("", None, noise_blanker=True)
    try:
        with pytest.raises(_lib.Ft8rxError, match="float_frames.*noise_blanker"):
            r.decode_frames(np.zeros((1, NSAMP), np.float32), float_frames=True)
        with pytest.raises(_lib.Ft8rxError, match="integers in int16 range"):
            Receiver("", None).decode_frames(np.zeros((1, NSAMP), np.float32))
    finally:
        r.close()
