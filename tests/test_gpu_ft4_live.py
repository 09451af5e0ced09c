"""Live FT4 on the GPU: ft8rx_ddc_stream_frames against the ring's own bytes, a live receiver on an FT4-only
stream and on a stream with an FT8 and an FT4 channel -- each held to decode_frames_ft4 on the very samples the ring held (the same
kernels on the same samples) -- and what must not have moved: a receiver without `modes`, and FT8 on a handle that has run FT4 live.
The inputs are tests/ft4_live_cases.py's; tests/test_ft4_live.py checks their premise on the float64 twin."""
import threading
import time as _t

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import ddc_stream_cases as live8
import ft4_live_cases as L4
from conftest import load_golden
from pyft8_amd import _lib, ddc
from pyft8_amd.receiver import Receiver
from test_gpu_ddc_stream import SRC, dials, iq

pytestmark = pytest.mark.gpu

NSAMP, SLOT = 180000, 90000


def text(d):
    return " ".join(d["msg_tuple"])


def stamp(t):
    return _t.strftime("%y%m%d_%H%M%S", _t.gmtime(int(np.floor(t))))


# ---- 1. the gather
def test_gather():
    """ft8rx_ddc_stream_frames against ft8rx_ddc_stream_read byte for byte on the stream of tests/test_gpu_ddc_stream.py: test_gather
    (24 kHz IQ int16, three channels): both frame lengths; a list, a list of repeats, NULL; odd and negative m_first; n_have 0, 1, 72000
    and full; a range that wraps the ring, the oldest range held and one sample older; every refusal with its word.  FT4's workspaces
    appear with the first 90000-sample call that names no buffer; ft8rx_ddc_stream_frame gives the bytes it gave."""
    rate = 24000
    x = iq(rate, 11)
    handle = _lib.Handle(device=0, max_frames=3)
    try:
        handle.ddc_stream_open(ddc.IQ_I16, rate, 2, SRC, dials(rate))
        for _ in range(3):
            m = handle.ddc_stream_push(x)
        assert 30000 < m < 36000

        def old_frames(m_first, n_have):
            handle.ddc_stream_frame(m_first, n_have)
            return handle.download_audio(handle.staging_ptr(), 3)

        def frames(m_first, n_have, frame_len, channels, n_sel=None):
            handle.ddc_stream_frames(m_first, n_have, frame_len, channels, n_sel)
            ch = list(range(3 if n_sel is None else n_sel)) if channels is None else list(channels)
            got = (handle.download_audio(handle.staging_ptr(), len(ch)) if frame_len == NSAMP else
                   handle.download_audio_ft4(handle.ft4_staging_ptr(), len(ch)))
            want = np.zeros((len(ch), frame_len), np.int16)
            lo, hi = max(m_first, 0), min(m_first + n_have, m)
            if hi > lo:
                want[:, lo - m_first:hi - m_first] = handle.ddc_stream_read(lo, hi - lo)[ch]
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), (m_first, n_have, frame_len, channels)
            return got

        before = [old_frames(1001, NSAMP), old_frames(-6001, NSAMP), old_frames(2000, 5000)]
        lists = ([2, 0], [1, 1, 1], None)
        for ch in lists:                                                               # 15-s frames first: nothing of FT4 exists yet
            a = frames(1001, NSAMP, NSAMP, ch)
            assert a[:, :m - 1001].std() > 1000 and not a[:, m - 1001:].any()
        assert handle.ft4_info()["workspace_bytes"] == 0 and handle.ft4_staging_ptr() == 0
        a = frames(1001, SLOT, SLOT, [2, 0])
        assert handle.ft4_info()["workspace_bytes"] > 0 and handle.ft4_staging_ptr() != 0 and a[:, :m - 1001].std() > 1000
        for frame_len in (SLOT, NSAMP):
            for ch in lists:
                a = frames(-6001, frame_len, frame_len, ch)                            # before the origin: a zero head
                assert not a[:, :6001].any() and a[:, 6001:6001 + m].std() > 1000
                for n_have in (0, 1, 5000, 72000):                                     # below a frame: a zero tail
                    a = frames(2001, n_have, frame_len, ch)
                    assert not a[:, n_have:].any() and (n_have < 2 or a[:, :min(n_have, m - 2001)].std() > 1000)
                frames(-frame_len - 5, frame_len, frame_len, ch)                       # nothing of it exists: zeros
            assert frames(1001, frame_len, frame_len, None, n_sel=2).shape == (2, frame_len)      # NULL = channels 0 .. n_sel - 1
        # a list is a list: [2, 0] is rows 2 and 0 of the old entry's frames, and repeats are copies
        assert frames(1001, NSAMP, NSAMP, [2, 0]).tobytes() == before[0][[2, 0]].tobytes()
        a = frames(2000, 5000, NSAMP, [1, 1, 1])
        assert a[0].tobytes() == a[1].tobytes() == a[2].tobytes() == before[2][1].tobytes()
        for _ in range(29):
            m = handle.ddc_stream_push(x)
        assert 2 * NSAMP + 20000 < m < 2 * NSAMP + 24000
        for frame_len in (SLOT, NSAMP):
            for ch in lists:
                a = frames(2 * NSAMP - 9999, 30000, frame_len, ch)                     # wraps the output ring
                assert a[:, :30000].std() > 1000
                a = frames(m - 2 * NSAMP, frame_len, frame_len, ch)                    # the oldest outputs the ring holds
                assert a.std() > 1000
                with pytest.raises(_lib.Ft8rxError, match="left the ring"):
                    handle.ddc_stream_frames(m - 2 * NSAMP - 1, frame_len, frame_len, ch)
                with pytest.raises(_lib.Ft8rxError, match="left the ring"):
                    handle.ddc_stream_frames(-6000, frame_len, frame_len, ch)
        for args, word in (((m - 1000, 1000, 1000, [0]), "frame_len 1000"), ((m - 1000, SLOT + 1, SLOT, [0]), "n_have"),
                           ((m - 1000, NSAMP + 1, NSAMP, [0]), "n_have"), ((m - 1000, -1, SLOT, None), "n_have"),
                           ((m - 1000, SLOT, SLOT, [0, 3]), "channel 3"), ((m - 1000, SLOT, SLOT, [-1]), "channel -1"),
                           ((m - 1000, SLOT, SLOT, []), "n_sel 0"), ((m - 1000, SLOT, SLOT, [0, 1, 2, 0]), "n_sel 4"),
                           ((m - 1000, SLOT, SLOT, None, 0), "n_sel 0")):
            with pytest.raises(_lib.Ft8rxError, match=word):
                handle.ddc_stream_frames(*args)
        # the old entry after all of it: the bytes it gave before, and the ring's
        a = old_frames(2 * NSAMP - 9999, 30000)
        assert a[:, :30000].tobytes() == handle.ddc_stream_read(2 * NSAMP - 9999, 30000).tobytes() and not a[:, 30000:].any()
        handle.ddc_stream_close()
        with pytest.raises(_lib.Ft8rxError, match="no stream is open"):
            handle.ddc_stream_frames(0, SLOT, SLOT, [0])
        handle.ddc_stream_open(ddc.IQ_I16, rate, 2, SRC, dials(rate))                   # a new stream: a table of its own
        for _ in range(3):
            handle.ddc_stream_push(x)
        assert old_frames(1001, NSAMP).tobytes() == before[0].tobytes() and old_frames(-6001, NSAMP).tobytes() == before[1].tobytes()
        m = handle.ddc_stream_info()["m_produced"]
        frames(1001, SLOT, SLOT, [2, 0])
    finally:
        handle.close()


# ---- 2. live, FT4 only
class Spy:
    """Counts and records on a live handle: the gathers of either entry, and the results of every FT4 batch with the n_have it saw"""
    def __init__(self, h):
        self.frames_calls, self.frame_calls, self.ft4 = [], 0, []
        frames, frame, fetch, enqueue = h.ddc_stream_frames, h.ddc_stream_frame, h.fetch, h.ft4_enqueue

        def w_frames(m_first, n_have, frame_len, channels=None, *a, **kw):
            self.frames_calls.append((m_first, n_have, frame_len, None if channels is None else tuple(channels)))
            return frames(m_first, n_have, frame_len, channels, *a, **kw)

        def w_frame(*a, **kw):
            self.frame_calls += 1
            return frame(*a, **kw)

        def w_enqueue(ptr, B):
            self.pending = self.frames_calls[-1]
            return enqueue(ptr, B)

        def w_fetch(B, *a, **kw):
            res = fetch(B, *a, **kw)
            if getattr(self, "pending", None) is not None:
                self.ft4.append((self.pending, res))
                self.pending = None
            return res
        h.ddc_stream_frames, h.ddc_stream_frame, h.fetch, h.ft4_enqueue = w_frames, w_frame, w_fetch, w_enqueue


def run_live(x, rate, t_first, spy=True, **kw):
    """The stream pushed in chunks of 1920 / 1000 with a poll() after each on a virtual clock, then flush() -> (the receiver, still
    open; [(samples pushed when it arrived, dict)]; the Spy on its live handle)"""
    vt, pushed, got = [t_first], [0], []
    rx = Receiver("x", lambda d: got.append((pushed[0], d)), time_source=lambda: vt[0], sample_rate=rate, iq=True, t_first=t_first, **kw)
    s = None
    try:
        returned = []
        for chunk, n in L4.live_chunks(x):
            pushed[0], vt[0] = n, t_first + n / rate
            rx.wide_in.push(chunk)
            if s is None and spy:
                s = Spy(rx._live)
            returned += rx.poll()
        rx.wide_in.flush()
        returned += rx.poll()
        assert returned == [d for _, d in got]                                          # poll() returns what on_message saw
    except BaseException:
        rx.stop()
        raise
    return rx, got, s


def control(rx, ctl, m_first, channel):
    """decode_frames_ft4 on the 90000 outputs from m_first on, as the live receiver's ring holds them"""
    y = rx._live.ddc_stream_read(m_first, SLOT)[channel]
    out, rec, cnt = ctl.decode_frames_ft4(y[None], return_records=True)
    return out[0], rec[0][:int(cnt[0])]


@pytest.fixture(scope="module")
def ft4_only():
    """The FT4-only session, run once: per slot the delivered (n, dict) list, the control's dicts and records, the live complete pass's
    records; and an FT8 decode_batch on the live handle after the session against a fresh handle's"""
    x, rate = L4.stream_ft4(), L4.RATE
    rx, got, spy = run_live(x, rate, L4.T_FIRST, dial_offsets_hz=(L4.DIAL,), bands=(L4.BAND,), modes="FT4")
    ctl = Receiver("", None, max_frames=1)
    try:
        assert rx.wide_in.modes == ("FT4",) and rx._live.max_frames == 1 and rx.ft4_early_samples == (72000,)
        ctls = [control(rx, ctl, SLOT * c, 0) for c in range(3)]
        audio = load_golden("test_08")[0][None]
        after = rx._live.decode_batch(audio)
        fresh_h = _lib.Handle(rx.cfg, device=0, max_frames=1)
        fresh_h.set_ladder_mode(1)
        fresh = fresh_h.decode_batch(audio)
        fresh_h.close()
    finally:
        rx.stop()
        ctl.close()
    return dict(got=got, ctls=ctls, spy=spy, after=after, fresh=fresh, call_hashes=rx.call_hashes)


def by_slot(got, n_slots, c0=1000, t_slot=7.5):
    cs = [stamp(t_slot * (c0 + c)) for c in range(n_slots)]
    out = [[] for _ in range(n_slots)]
    for n, d in got:
        out[cs.index(d["cyclestart_string"])].append((n, d))
    return out


def test_live_ft4_only(ft4_only):
    """Three slots (make_frame 12 and 17, noise) at one dial of a 48 kHz IQ stream.  Per slot the delivered texts are the control's, none
    twice, with channel, band, slot start, parity and mode; nothing from the noise slot; every early message arrived before the slot's
    last sample was pushed and every other one after; slot 0 has the early rows the twin pins and something late; the complete pass's
    records are the control's byte for byte."""
    got, ctls, spy = ft4_only["got"], ft4_only["ctls"], ft4_only["spy"]
    per_slot = SLOT * L4.RATE // 12000
    slots = by_slot(got, 3)
    for c, lst in enumerate(slots):
        texts = [text(d) for _, d in lst]
        want = [text(d) for d in ctls[c][0]]
        print(f"live FT4 slot {c}: {len(texts)} messages, {sum(d['early'] for _, d in lst)} early; control {len(want)}")
        assert len(set(texts)) == len(texts) and set(texts) == set(want), (c, sorted(texts), sorted(want))
        for n, d in lst:
            assert d["mode"] == "FT4" and d["channel"] == 0 and d["band"] == L4.BAND and d["their_tx_cycle"] == (1000 + c) % 2
            assert d["cyclestart_string"] == stamp(7.5 * (1000 + c)) and 0.0 < d["fHz"] < 3000.0 and d["all_txt_format"].startswith(d["cyclestart_string"])
            assert (n < per_slot * (c + 1)) if d["early"] else (n >= per_slot * (c + 1)), (c, n, d["early"])
    assert len(slots[0]) >= 6 and len(slots[1]) >= 1 and slots[2] == [] and ctls[2][0] == []
    assert sum(d["early"] for _, d in slots[0]) >= 4 and sum(not d["early"] for _, d in slots[0]) >= 1
    # the four signals the twin finds at rows 34 .. 59 (tests/test_ft4_live.py: the earliest four starts) came early, by construction
    assert set(L4.texts_by_start(12)[:4]) <= {text(d) for _, d in slots[0] if d["early"]}
    # the passes that ran: (c, 72000) then (c, 90000) per slot, each once, channel 0
    assert [p for p, _ in spy.ft4] == [(SLOT * c, n, SLOT, (0,)) for c in range(3) for n in (72000, SLOT)] and spy.frame_calls == 0
    for c in range(3):
        (_, (rec, cnt, _, _)), want = spy.ft4[2 * c + 1], ctls[c][1]
        assert int(cnt[0]) == len(want) and rec[0][:len(want)].tobytes() == want.tobytes(), c


def test_ft8_after_live_ft4(ft4_only):
    """An FT8 decode_batch on the handle that ran the FT4 session equals a fresh handle's: counts, and the records they cover"""
    a, f = ft4_only["after"], ft4_only["fresh"]
    assert a[1].tobytes() == f[1].tobytes() and int(f[1][0]) > 0 and a[3].tobytes() == f[3].tobytes()
    assert a[0][0, :int(f[1][0])].tobytes() == f[0][0, :int(f[1][0])].tobytes()


def test_live_ft4_subtraction_passes(ft4_only):
    """ft4_passes = 2 on a second receiver over the same stream: per slot pass 1's messages unchanged at the head, in order, then the
    later pass's with _SUB in their notes; never fewer texts, none twice; the later pass runs on the complete slot only"""
    rx, got, spy = run_live(L4.stream_ft4(), L4.RATE, L4.T_FIRST, dial_offsets_hz=(L4.DIAL,), bands=(L4.BAND,), modes="FT4", ft4_passes=2)
    rx.stop()
    one, two = by_slot(ft4_only["got"], 3), by_slot(got, 3)
    per_slot = SLOT * L4.RATE // 12000
    for c in range(3):
        t1, t2 = [text(d) for _, d in one[c]], [text(d) for _, d in two[c]]
        print(f"live FT4 slot {c}: {len(t1)} messages with one pass, {len(t2)} with two")
        assert t2[:len(t1)] == t1 and len(set(t2)) == len(t2)
        assert [(d["early"], d["decode_notes"]) for _, d in two[c][:len(t1)]] == [(d["early"], d["decode_notes"]) for _, d in one[c]]
        assert all("_SUB" in d["decode_notes"] and not d["early"] and n >= per_slot * (c + 1) for n, d in two[c][len(t1):])
        assert all("_SUB" not in d["decode_notes"] for _, d in two[c][:len(t1)])
    n_batches = [sum(1 for p, _ in spy.ft4 if p[:2] == (SLOT * c, n)) for c in range(3) for n in (72000, SLOT)]
    assert n_batches[0::2] == [1, 1, 1] and all(n >= 1 for n in n_batches[1::2])     # early passes are single


def test_live_ft4_subtraction_passes_find_more():
    """Two crowded slots (16 signals in 900 Hz each; the twin's second pass finds more, tests/test_ft4_sub.py) with ft4_passes = 1 and 2:
    the two-pass receiver delivers per slot the texts of decode_frames_ft4 with two passes on the very samples the ring held, pass 1's at
    the head as the one-pass receiver delivered them, the later pass's behind them with _SUB, after the slot's last sample, none twice"""
    kw = dict(dial_offsets_hz=(L4.DIAL,), bands=(L4.BAND,), modes="FT4", max_cands=L4.CROWDED_MAX_CANDS)
    x, per_slot = L4.stream_crowded(), SLOT * L4.RATE // 12000
    rx1, got1, _ = run_live(x, L4.RATE, L4.T_FIRST, **kw)
    rx1.stop()
    rx2, got2, spy = run_live(x, L4.RATE, L4.T_FIRST, ft4_passes=2, **kw)
    ctl = Receiver("", None, max_frames=1, max_cands=L4.CROWDED_MAX_CANDS, ft4_passes=2)
    try:
        want = [[text(d) for d in ctl.decode_frames_ft4(rx2._live.ddc_stream_read(SLOT * c, SLOT)[0][None])[0]] for c in range(2)]
    finally:
        rx2.stop()
        ctl.close()
    one, two = by_slot(got1, 2), by_slot(got2, 2)
    planted = [{t["msg"] for t in L4.sub4.crowded(i)[1]} for i in L4.CROWDED]
    n_sub = 0
    for c in range(2):
        t1, t2 = [text(d) for _, d in one[c]], [text(d) for _, d in two[c]]
        sub = two[c][len(t1):]
        print(f"crowded live slot {c}: {len(t1)} messages with one pass, {len(t2)} with two ({sum(d['early'] for _, d in two[c])} early); control {len(want[c])}")
        assert t2[:len(t1)] == t1 and len(set(t2)) == len(t2)
        # the complete slot's passes are the control's (the same kernels on the same samples).  An early pass searches a grid whose tail
        # is zero, so it may find a candidate the complete slot's search does not: such a text is early, and one that was planted
        extra = set(t2) - set(want[c])
        assert set(want[c]) <= set(t2) and extra <= {text(d) for _, d in two[c] if d["early"]} and extra <= planted[c], (c, extra)
        assert all("_SUB" not in d["decode_notes"] for _, d in two[c][:len(t1)])
        assert all("_SUB" in d["decode_notes"] and not d["early"] and n >= per_slot * (c + 1) and d["channel"] == 0 and d["band"] == L4.BAND
                   and d["their_tx_cycle"] == c % 2 for n, d in sub)
        n_sub += len(sub)
    assert n_sub >= 1                                                                   # the later pass had something to find
    assert [sum(1 for p, _ in spy.ft4 if p[:2] == (SLOT * c, 72000)) for c in range(2)] == [1, 1]      # early passes are single
    assert all(sum(1 for p, _ in spy.ft4 if p[:2] == (SLOT * c, SLOT)) == 2 for c in range(2))


# ---- 3. an FT8 and an FT4 channel on one stream
def test_live_mixed(monkeypatch):
    """One 15-s 48 kHz IQ stream: channel 0 an FT8 cycle of tests/ddc_stream_cases.py, channel 1 two FT4 slots, modes=("FT8", "FT4").
    Channel 0 delivers that frame's six texts, channel 1 its control's; both are packaged with the receiver's one call-hash table; the
    same stream from an iterator through the daemon thread delivers the same."""
    x, rate, offs, t_first = L4.stream_mixed(), L4.RATE, live8.offsets(), 15.0 * 1000
    tables = []
    for name in ("package_batch", "package_batch_ext"):
        fn = getattr(_lib, name)
        monkeypatch.setattr(_lib, name, lambda *a, _fn=fn, **kw: (tables.append(kw.get("table")), _fn(*a, **kw))[1])
    kw = dict(dial_offsets_hz=offs, bands=L4.MIXED_BANDS, modes=("FT8", "FT4"))
    rx, got, spy = run_live(x, rate, t_first, **kw)
    ctl = Receiver("", None, max_frames=1)
    try:
        assert rx._live.max_frames == 2 and rx.wide_in.channels == {"FT8": [0], "FT4": [1]}
        assert len(tables) >= 6 and all(t is rx.call_hashes for t in tables)           # FT8 and FT4 passes alike: the one table
        ctls = [control(rx, ctl, SLOT * c, 1) for c in range(2)]
    finally:
        rx.stop()
        ctl.close()
    want8 = live8.messages(L4.MIXED_FT8)[0]
    ft8 = [(n, d) for n, d in got if d["channel"] == 0]
    texts8 = [text(d) for _, d in ft8]
    assert len(set(texts8)) == len(texts8) and set(texts8) == want8
    assert all(d.get("mode", "FT8") == "FT8" and d["band"] == "20m" and d["cyclestart_string"] == stamp(t_first) for _, d in ft8)
    assert any(d["early"] for _, d in ft8)
    ft4 = by_slot([(n, d) for n, d in got if d["channel"] == 1], 2, c0=2000)
    for c, lst in enumerate(ft4):
        texts = [text(d) for _, d in lst]
        want = [text(d) for d in ctls[c][0]]
        print(f"mixed stream, FT4 slot {c}: {len(texts)} messages, {sum(d['early'] for _, d in lst)} early; control {len(want)}")
        assert len(set(texts)) == len(texts) and set(texts) == set(want) and len(texts) >= 1
        assert all(d["mode"] == "FT4" and d["band"] == "20m-ft4" and d["their_tx_cycle"] == c % 2 for _, d in lst)
    # the gathers: FT8's with its list at 180000, FT4's with its list at 90000, the old entry not at all
    assert spy.frame_calls == 0 and {p[2:] for p in spy.frames_calls} == {(NSAMP, (0,)), (SLOT, (1,))}
    assert [p[:2] for p in spy.frames_calls if p[2] == SLOT] == [(SLOT * c, n) for c in range(2) for n in (72000, SLOT)]

    # the same stream from an iterator: the constructor opens the source and starts the daemon (virtual clock and sleep seams)
    vt, lock, got2, box = [t_first], threading.Lock(), [], []

    def source():
        # (the wait-for-_ready seam of tests/test_gpu_ddc_stream.py: test_live_end_to_end)
        for chunk, n in L4.live_chunks(x):
            with lock:
                vt[0] = t_first + n / rate
            yield chunk
            while box and box[0].wide_in._ready and box[0].thread_error is None and box[0]._thread.is_alive():
                _t.sleep(0.0005)

    rx = Receiver("x", got2.append, time_source=lambda: vt[0], sleep=lambda dt: _t.sleep(0.002), audio_source=source(), sample_rate=rate,
                  iq=True, t_first=t_first, **kw)
    box.append(rx)
    try:
        assert rx._thread is not None and rx._thread.is_alive()
        deadline = _t.time() + 120
        while not (rx.wide_in.source_exhausted and not rx.wide_in._ready) and rx.thread_error is None and _t.time() < deadline:
            _t.sleep(0.02)
    finally:
        rx.stop()
    assert rx.thread_error is None and rx.wide_in.source_exhausted

    def key(d):
        return (d["cyclestart_string"], d["channel"], d["band"], d.get("mode", "FT8"), text(d))
    assert sorted(key(d) for d in got2) == sorted(key(d) for _, d in got)


# ---- 4. nothing else moved
def test_without_modes_nothing_new_is_called():
    """The stream of test_live_end_to_end through a receiver without `modes`, and with every channel "FT8": no call of the new entry, the
    old one for every pass, and per cycle and channel the six texts"""
    x, offs, rate, t_first = live8.stream(), live8.offsets(), live8.RATE, 15.0 * 1000
    want = {(c, j): live8.messages(live8.PLAN[c][j])[0] for c in range(2) for j in range(2)}
    results = []
    for kw in ({}, {"modes": ("FT8", "FT8")}):
        rx, got, spy = run_live(x, rate, t_first, dial_offsets_hz=offs, bands=live8.BANDS, **kw)
        rx.stop()
        assert rx.wide_in.modes is None and spy.frames_calls == [] and spy.frame_calls == 6 and spy.ft4 == []
        by = {k: set() for k in want}
        for _, d in got:
            c = [stamp(t_first + 15 * c) for c in range(2)].index(d["cyclestart_string"])
            assert text(d) not in by[(c, d["channel"])] and d.get("mode", "FT8") == "FT8"
            by[(c, d["channel"])].add(text(d))
        assert by == want
        results.append([(n, d["cyclestart_string"], d["channel"], d["early"], text(d)) for n, d in got])
    assert results[0] == results[1]
