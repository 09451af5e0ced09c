"""ft8rx_blank (csrc/kernels/blanker.hpp) against its numpy twin, bit for bit, on the crafted frames of
tests/blanker_cases.py; Receiver(noise_blanker=) wherever frames are decoded.  Run with -m gpu on an MI355X."""
import ctypes as C
import threading
import time as _t

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import blanker_cases as cases
import oracle as O
from pyft8_amd import _lib, blanker
from pyft8_amd.receiver import Receiver, decode_frames

pytestmark = pytest.mark.gpu
NSAMP = cases.NSAMP
SENTINEL = (np.arange(NSAMP) % 30011 - 15000).astype(np.int16)           # loud everywhere: any stray gate or write would show


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle(max_frames=4)
    yield h
    h.close()


def _same(got, ref, what):
    y, stats, lv = ref
    gy, gs, gl = got
    assert np.array_equal(gs, stats), (what, gs, stats)
    if gl is not None:
        assert np.array_equal(gl, lv), what
    assert gy.tobytes() == y.tobytes(), (what, np.flatnonzero((gy != y).any(axis=0))[:8])


@pytest.mark.parametrize("k,guard,taper", cases.PARAM_SETS)
def test_blank_is_the_twin_bit_for_bit(handle, k, guard, taper):
    """B = 3 on a handle of max_frames 4: y, stats and levels on a caller's device buffer, on the staging audio, through
    ft8rx_blank_host; the fourth frame, a sentinel, keeps its bytes."""
    q8 = blanker.check(k, guard, taper)[0]
    bs, refs = cases.batches(k, guard, taper)
    dev = torch.device("cuda", 0)
    for i, (x, ref) in enumerate(zip(bs, refs)):
        four = np.concatenate([x, SENTINEL[None]])
        # a caller's device buffer
        d = torch.from_numpy(four.copy()).to(dev)
        torch.cuda.synchronize(dev)
        stats, lv = handle.blank(d.data_ptr(), 3, q8, guard, taper, want_levels=True)
        got = d.cpu().numpy()
        _same((got[:3], stats, lv), ref, ("device", i))
        assert got[3].tobytes() == SENTINEL.tobytes()
        # the staging audio (filled by a batch of four), d_audio = NULL
        handle.decode_batch(four)
        stats, lv = handle.blank(None, 3, q8, guard, taper, want_levels=True)
        got = handle.download_audio(handle.staging_ptr(), 4)
        _same((got[:3], stats, lv), ref, ("staging", i))
        assert got[3].tobytes() == SENTINEL.tobytes()
        # from host memory
        stats = handle.blank_host(x, q8, guard, taper)
        _same((handle.download_audio(handle.staging_ptr(), 3), stats, None), ref, ("host", i))
    # queued only (no stats, no levels): the next call on the handle sees the result
    d = torch.from_numpy(bs[0].copy()).to(dev)
    torch.cuda.synchronize(dev)
    assert handle.blank(d.data_ptr(), 3, q8, guard, taper, want_stats=False) is None
    handle.sync()
    assert d.cpu().numpy().tobytes() == refs[0][0].tobytes()


def test_blank_on_a_buffer_that_is_only_sample_aligned(handle):
    """2 bytes past a 16-byte boundary the kernels take the 2-byte path: the same bits, and nothing outside the frames is written"""
    k, guard, taper = cases.PARAM_SETS[2]
    q8 = blanker.check(k, guard, taper)[0]
    bs, refs = cases.batches(k, guard, taper)
    dev = torch.device("cuda", 0)
    buf = np.full(3 * NSAMP + 16, 12345, np.int16)
    buf[1:1 + 3 * NSAMP] = bs[1].reshape(-1)
    d = torch.from_numpy(buf).to(dev)
    torch.cuda.synchronize(dev)
    assert d.data_ptr() % 16 == 0
    stats, lv = handle.blank(d.data_ptr() + 2, 3, q8, guard, taper, want_levels=True)
    got = d.cpu().numpy()
    _same((got[1:1 + 3 * NSAMP].reshape(3, NSAMP), stats, lv), refs[1], "unaligned")
    assert got[0] == 12345 and (got[1 + 3 * NSAMP:] == 12345).all()


def test_refusals_name_the_argument(handle):
    L, h = handle._L, handle._h
    x = np.zeros((1, NSAMP), np.int16)
    for args, name in (((5, 2048, 6, 6), "n_frames"), ((0, 2048, 6, 6), "n_frames"), ((1, 511, 6, 6), "threshold_q8"), ((1, 16385, 6, 6), "threshold_q8"),
                       ((1, 2048, 65, 6), "guard"), ((1, 2048, -1, 6), "guard"), ((1, 2048, 6, -1), "taper"), ((1, 2048, 6, 65), "taper")):
        assert L.ft8rx_blank(h, None, *args, None, None) == -1
        assert name in L.ft8rx_last_error(h).decode()
        assert L.ft8rx_blank_host(h, x.ctypes.data, *args, None) == -1
        assert name in L.ft8rx_last_error(h).decode()
    assert L.ft8rx_blank(h, C.c_void_p(handle.staging_ptr() + 1), 1, 2048, 6, 6, None, None) == -1
    assert "d_audio" in L.ft8rx_last_error(h).decode()
    assert L.ft8rx_blank_host(h, None, 1, 2048, 6, 6, None) == -1 and "audio" in L.ft8rx_last_error(h).decode()
    # the limits themselves are taken
    assert L.ft8rx_blank_host(h, x.ctypes.data, 1, 512, 0, 0, None) == 0 and L.ft8rx_blank_host(h, x.ctypes.data, 1, 16384, 64, 64, None) == 0


def _fields(d):
    return (" ".join(d["msg_tuple"]), d["their_snr"], d["fHz"], d["tsec"], d["decode_notes"])


@pytest.fixture(scope="module")
def recipe_decodes():
    """(noisy frames, what Receiver(noise_blanker=True).decode_frames returns for them)"""
    _, noisy, _ = cases.recipe()
    rx = Receiver("", None, max_frames=3, noise_blanker=True)
    try:
        out = rx.decode_frames(noisy)
        stats = rx.blanker_stats.copy()
    finally:
        rx.close()
    return noisy, out, stats


def test_receiver_decodes_what_the_oracle_decodes_behind_the_twin(recipe_decodes):
    """Frame for frame: text, emit order, snr / fHz / tsec and the decode notes of oracle.decode_frame(blanker.reference(noisy)); a
    receiver without the option returns what the plain decode of the noisy frames returns."""
    noisy, got, stats = recipe_decodes
    blanked, want_stats, _ = blanker.reference(noisy)
    assert np.array_equal(stats, want_stats) and (stats[:, 0] > 1000).all()
    ocfg = O.default_config(**_lib.fft_plans())
    n = 0
    for f in range(len(noisy)):
        want = O.decode_frame(blanked[f], ocfg)["msgs"]
        assert [" ".join(d["msg_tuple"]) for d in got[f]] == [" ".join(m["msg_tuple"]) for m in want]
        for d, m in zip(got[f], want):
            assert d["their_snr"] == f"{m['snr']:+03d}" and abs(d["tsec"] - m["tsec"]) < 1e-9 and abs(d["fHz"] - m["fHz"]) < 1e-9
            assert d["decode_notes"] == O.notes_of(m)
        n += len(want)
    assert n >= 50
    # off: today's path, today's result
    rx = Receiver("", None, max_frames=3)
    try:
        off = rx.decode_frames(noisy)
        assert rx.blanker_stats is None and rx.noise_blanker is None
        rec, cnt, ev, evc = rx._handle(3).decode_batch(noisy)
    finally:
        rx.close()
    msgs, mcnt = _lib.package_batch(rec, cnt, ev, evc)
    for f in range(len(noisy)):
        want = O.decode_frame(noisy[f], ocfg)["msgs"]
        assert [" ".join(d["msg_tuple"]) for d in off[f]] == [" ".join(m["msg_tuple"]) for m in want]
        assert int(mcnt[f]) == len(want)
    assert sum(len(o) for o in off) < n - 20
    # the module-level function passes the option through; a threshold and a dict are taken
    one = decode_frames(noisy[:1], noise_blanker=True)
    assert [_fields(d) for d in one[0]] == [_fields(d) for d in got[0]]
    also = decode_frames(noisy[:1], noise_blanker={"threshold": 8.0, "guard": 6, "taper": 6})
    assert [_fields(d) for d in also[0]] == [_fields(d) for d in got[0]]


def test_passes_and_arrays_blank_once_before_the_first_pass(recipe_decodes):
    noisy, got, stats = recipe_decodes
    rx = Receiver("", None, max_frames=3, noise_blanker=True)
    try:
        two = rx.decode_frames(noisy, passes=2)
        assert np.array_equal(rx.blanker_stats, stats)
        msgs, mcnt, rec, cnt = rx.decode_frames_arrays(noisy)
        assert np.array_equal(rx.blanker_stats, stats)
    finally:
        rx.close()
    for f in range(len(noisy)):
        first = [_fields(d) for d in two[f][:len(got[f])]]
        assert first == [_fields(d) for d in got[f]]                                  # the first pass is the single pass
        assert all(d["decode_notes"].endswith("_SUB") for d in two[f][len(got[f]):])
        assert int(mcnt[f]) == len(got[f])


def test_decode_stream_blanks_behind_the_down_converter():
    """48 kHz real input with bursts: the staging frames after the call are the twin applied to the down-converter's frames"""
    rng = np.random.default_rng(5)
    x = np.rint(1000.0 * rng.standard_normal(15 * 48000))
    for p in rng.integers(1000, 15 * 48000 - 1000, 200):
        x[p:p + 4] += 30000.0 * rng.choice([-1.0, 1.0])
    x = np.clip(x, -32768, 32767).astype(np.int16)
    off = Receiver("", None, max_frames=1)
    on = Receiver("", None, max_frames=1, noise_blanker=True)
    try:
        off.decode_stream(x, 48000)
        plain = off._h.download_audio(off._h.staging_ptr(), 1)
        on.decode_stream(x, 48000)
        got = on._h.download_audio(on._h.staging_ptr(), 1)
        stats = on.blanker_stats
    finally:
        off.close()
        on.close()
    y, want_stats, _ = blanker.reference(plain)
    assert np.array_equal(stats, want_stats) and stats[0, 0] >= 100
    assert got.tobytes() == y.tobytes() and got.tobytes() != plain.tobytes()


def test_live_cycle_through_audio_source(recipe_decodes):
    """One cycle of hops under the virtual clock, impulses added: the delivered messages are decode_frames' with the option on the same
    frame; an early pass (a partial cycle, zero behind it) is blanked as well."""
    noisy, got_batch, _ = recipe_decodes
    audio = noisy[0]
    want = [_fields(d) for d in got_batch[0]]
    vt, lock, got = [0.0], threading.Lock(), []

    def hops():
        for k in range(375):
            with lock:
                vt[0] = (k + 1) * 0.04
            yield audio[480 * k:480 * k + 480]

    rx = Receiver("any", got.append, time_source=lambda: vt[0], sleep=lambda dt: _t.sleep(0.002), audio_source=hops(), early_decode_hop=None,
                  noise_blanker=True)
    try:
        deadline = _t.time() + 60
        while len(got) < len(want) and rx.thread_error is None and _t.time() < deadline:
            _t.sleep(0.01)
    finally:
        rx.stop()
    assert rx.thread_error is None
    assert [_fields(d) for d in got] == want
    assert np.array_equal(rx.blanker_stats, blanker.reference(audio)[1])
    # an early pass, fed by hand: 320 hops, then poll
    rx = Receiver("x", None, time_source=lambda: vt[0], autostart=False, early_decode_hop=320, noise_blanker=True)
    try:
        rx.audio_in.search_grid_ptr = 0
        for k in range(320):
            vt[0] = (k + 1) * 0.04
            rx.audio_in._callback(audio[480 * k:480 * k + 480].tobytes())
        early = rx.poll()
        part = np.zeros(NSAMP, np.int16)
        part[:320 * 480] = audio[:320 * 480]
        assert np.array_equal(rx.blanker_stats, blanker.reference(part)[1]) and rx.blanker_stats[0, 3] == 55
        assert all(d["early"] for d in early)
    finally:
        rx.close()
