"""Live FT4 without a GPU: the FT4 pass scheduler and the mixed order of two schedulers on one sample clock, the
early-pass rule, the premise of the GPU test on the float64 twin (which of slot 0's signals an early pass may deliver), what the Python
surface refuses before a stream opens, the new symbol against the header, and the argument checks of ft8rx_ddc_stream_frames
(csrc/ddc_frames.hpp) under the host sanitizers."""
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

import ft4_live_cases as L4
from conftest import ROOT
from pyft8_amd import _abi, _lib, ft4, receiver, wide_in
from test_abi import c_prototypes, mismatches
from test_ddc_stream import expected_passes

NSAMP, SLOT, TILE = 180000, 90000, 1008


# ---- 1. the schedulers
def ft4_expected(t_first, early, m_end):
    """From the timing rule alone: slot c starts at m_c = round((7.5 c - t_first) 12000) and is decoded if m_c >= -6000; its passes are
    the early ones (n samples) and the complete slot (90000), each due once m_c + n_have outputs exist"""
    out = []
    c = int(t_first // 7.5) - 1
    while True:
        m_c = int(round((7.5 * c - t_first) * 12000))
        if m_c >= -6000:
            for n in tuple(early) + (SLOT,):
                if m_c + n > m_end:
                    return out
                out.append((c, n, m_c))
        c += 1


@pytest.mark.parametrize("t_first,first_slot,m_first", [(7.5 * 1000 + 0.3, 1000, -3600), (7.5 * 1000, 1000, 0), (7.5 * 1001, 1001, 0),
                                                          (7.5 * 1000 + 0.6, 1001, 82800)])
@pytest.mark.parametrize("early_s", [(6.0,), ()])
def test_ft4_scheduler(t_first, first_slot, m_first, early_s):
    """m_produced climbs in whole tiles of 1008: every pass is handed out exactly once, at the first step at which its outputs exist --
    (c, 72000) then (c, 90000) per slot, or with ft4_early_decode_s=() the complete slots alone"""
    early = wide_in.ft4_early_samples(early_s)
    assert early == ((72000,) if early_s else ())
    s = wide_in.ft4_scheduler(t_first, early)
    assert (s.cycle, s.cycle_start(s.cycle)) == (first_slot, m_first)
    for c in (first_slot, first_slot + 1, first_slot + 7):
        assert s.cycle_start(c) == int(round((7.5 * c - t_first) * 12000))             # m_c as defined
    got, m_end = [], 4 * SLOT
    for m in range(0, m_end + 1, TILE):
        for c, hop, m_c, n_have in s.due(m):
            assert m - TILE < m_c + n_have <= m and hop == (n_have if n_have < SLOT else 0)
            got.append((c, n_have, m_c))
    assert s.due(m_end // TILE * TILE) == []
    want = ft4_expected(t_first, early, m_end // TILE * TILE)
    assert got == want and len(set(got)) == len(got) and got[0][0] == first_slot and got[0][2] == m_first
    per_slot = [n for c, n, _ in got if c == first_slot + 1]
    assert per_slot == ([72000, SLOT] if early_s else [SLOT])


@pytest.mark.parametrize("t_first", [15014.2, 15000.4, 15000.5, 15000.6, 15000.0, 7.25])
def test_default_scheduler_is_unchanged(t_first):
    """The default-constructed PassScheduler on the inputs of tests/test_ddc_stream.py: test_scheduler gives the list it gave"""
    hops, D, total = (320, 340), 4, 35 * 48000
    s = wide_in.PassScheduler(t_first, hops)
    assert (s.period_s, s.n_samp, s.hop_len) == (15, NSAMP, 480)
    got, n, i, lens = [], 0, 0, (1920, 1000, 47999, 13, 48000, 1)
    while n < total:
        n = min(total, n + lens[i % len(lens)])
        i += 1
        got += s.due(wide_in.produced(n, D))
    assert got == expected_passes(t_first, hops, wide_in.produced(total, D)) and len(got) >= 3
    if t_first == 15014.2:
        assert got[:3] == [(1001, 320, 9600, 153600), (1001, 340, 9600, 163200), (1001, 0, 9600, NSAMP)]


class FakeHandle:
    def __init__(self, D):
        self.D, self.n = D, 0

    def ddc_stream_open(self, kind, rate, n_streams, src, dials):
        return np.zeros(len(src))

    def ddc_stream_push(self, a):
        self.n += a.shape[1]
        return wide_in.produced(self.n, self.D)


class FakeReceiver:
    def __init__(self, D):
        self.h, self._live_lock, self._stop = FakeHandle(D), threading.RLock(), threading.Event()
        self.early_decode_hops, self.ft4_early_samples, self.thread_error = (320,), (72000,), None
        self.time_source = lambda: 15000.0

    def _live_handle(self, n_frames=1):
        return self.h


def test_mixed_order():
    """An FT8 and an FT4 scheduler on one clock (WideIn(modes=...)): _ready carries the mode, ordered by the sample at which a pass falls
    due, FT8 before FT4 at a tie -- 15000.0 s is a boundary of both, so every FT8 cycle ends with an FT4 slot"""
    w = wide_in.WideIn(FakeReceiver(4), 48000, iq=True, dial_offsets_hz=(-1000.0, 2000.0, 5000.0), modes=("FT4", "FT8", "FT4"))
    assert w.modes == ("FT4", "FT8", "FT4") and w.channels == {"FT8": [1], "FT4": [0, 2]}
    x = np.ones((48000, 2), np.int16)
    seen = []
    for _ in range(16):
        w.push(x)
        assert w._ready[:len(seen)] == seen                                             # what is due stays in place: new passes follow
        seen = list(w._ready)
    w.flush()
    got = list(w._ready)
    assert got == [(2000, 72000, 0, 72000, "FT4"), (2000, 0, 0, SLOT, "FT4"), (1000, 320, 0, 153600, "FT8"), (2001, 72000, SLOT, 72000, "FT4"),
                   (1000, 0, 0, NSAMP, "FT8"), (2001, 0, SLOT, SLOT, "FT4")]
    due = [p[2] + p[3] for p in got]
    assert due == sorted(due) and due[4] == due[5]                                      # the tie: FT8 first
    assert wide_in.merge_due({"FT4": [(3, 0, 0, 90)], "FT8": [(1, 0, 0, 90), (2, 0, 10, 70)]}) == \
        [(2, 0, 10, 70, "FT8"), (1, 0, 0, 90, "FT8"), (3, 0, 0, 90, "FT4")]
    # without the keyword, and with every channel FT8, the entries are the four-tuples they were and no second scheduler exists
    for modes in (None, "FT8", ("FT8", "FT8")):
        w = wide_in.WideIn(FakeReceiver(4), 48000, iq=True, dial_offsets_hz=(-1000.0, 2000.0), **({} if modes is None else {"modes": modes}))
        assert w.modes is None and w.channels is None
        for _ in range(13):
            w.push(x)
        assert w._ready == [(1000, 320, 0, 153600)] and w.scheds is None
    w = wide_in.WideIn(FakeReceiver(4), 48000, iq=True, dial_offsets_hz=(-1000.0, 2000.0), modes="FT4")
    assert w.modes == ("FT4", "FT4") and w.channels == {"FT4": [0, 1]}


# ---- 2. the early rule
def test_early_rule():
    """144 h0 + 36 tt + 60480 + 144 <= n_have: both sides of the boundary in h0 and in tt, a negative start, the complete slot"""
    assert 144 * 79 + 60480 + 144 == 72000 == 144 * 78 + 36 * 4 + 60480 + 144           # (79, 0) and (78, +4) end on the last sample received
    assert ft4.early_ok(79, 0, 72000) and not ft4.early_ok(79, 0, 71999) and not ft4.early_ok(79, 1, 72000) and ft4.early_ok(79, 1, 72036)
    assert ft4.early_ok(78, 4, 72000) and not ft4.early_ok(78, 4, 71999)
    assert ft4.early_ok(80, -4, 72000) and not ft4.early_ok(80, -3, 72000) and not ft4.early_ok(80, 0, 72000)
    assert ft4.early_ok(-3, -4, 72000) and ft4.early_ok(-3, -4, 60048) and not ft4.early_ok(-3, -4, 60047)      # a start before the slot
    assert ft4.early_ok(204, 0, SLOT) and not ft4.early_ok(204, 1, SLOT)                # a late signal runs past the slot itself


def test_premise_of_the_gpu_test():
    """Slot 0 of the live test, zeroed from sample 72000 on, through the float64 twin: all six words, at the rows ROWS_12; the early rule
    admits four of them and not the other two, so the GPU test has early and late messages by construction"""
    x = np.array(L4.slot(12))
    x[L4.EARLY:] = 0
    words = L4.words(12)
    found = {d["word"]: d for d in ft4.decode_twin(x) if d["word"] is not None}
    assert set(found) == set(words) and len(words) == 6
    assert tuple(sorted(d["h0"] for d in found.values())) == L4.ROWS_12 == (34, 40, 49, 59, 86, 102)
    early = sorted(d["h0"] for d in found.values() if ft4.early_ok(d["h0"], d["tt"], L4.EARLY))
    assert early == [34, 40, 49, 59] and all(h0 <= 78 for h0 in early) and not any(ft4.early_ok(h0, -4, L4.EARLY) for h0 in (86, 102))
    # and the noise slot carries nothing
    assert all(d["word"] is None for d in ft4.decode_twin(np.array(L4.slot(None))))


def test_streams_of_the_cases():
    x = L4.stream_ft4()
    assert x.shape == (3 * SLOT * 4, 2) and x.dtype == np.int16 and np.abs(x.astype(np.int32)).max() < 32767
    y = L4.stream_mixed()
    assert y.shape == (NSAMP * 4, 2) and y.dtype == np.int16 and np.abs(y.astype(np.int32)).max() < 32767


# ---- 3. refusals that need no device
def test_modes_and_early_seconds_refusals():
    assert wide_in.channel_modes(None, 3) is None and wide_in.channel_modes("FT8", 3) is None and wide_in.channel_modes(["FT8"] * 2, 2) is None
    assert wide_in.channel_modes("FT4", 2) == ("FT4", "FT4") and wide_in.channel_modes(("FT8", "FT4"), 2) == ("FT8", "FT4")
    with pytest.raises(_lib.Ft8rxError, match=r"modes: one per channel \(2\), got 3"):
        wide_in.channel_modes(("FT8", "FT4", "FT4"), 2)
    with pytest.raises(_lib.Ft8rxError, match="modes: unknown mode 'FT2'"):
        wide_in.channel_modes(("FT8", "FT2"), 2)
    with pytest.raises(_lib.Ft8rxError, match="modes: unknown mode 'ft4'"):
        wide_in.channel_modes("ft4", 1)
    assert wide_in.ft4_early_samples((6.0,)) == (72000,) and wide_in.ft4_early_samples(()) == () and wide_in.ft4_early_samples(None) == ()
    assert wide_in.ft4_early_samples((6.5, 6.0, 6.0)) == (72000, 78000) and wide_in.ft4_early_samples(5.75) == (69000,)
    for bad in (0.0, 7.5, -1.0, 8.0, float("nan"), "6", True):
        with pytest.raises(_lib.Ft8rxError, match="ft4_early_decode_s: .* outside"):
            wide_in.ft4_early_samples((bad,))
    with pytest.raises(_lib.Ft8rxError, match="ft4_early_decode_s: .* whole number of 12 kHz samples"):
        wide_in.ft4_early_samples((6.00001,))


class NoDevice:
    """A handle that may be created and closed and nothing else: whatever the refusals below need, they need before a stream opens"""
    def __init__(self, cfg=None, device=0, max_frames=1):
        self.cfg, self.max_frames = cfg, int(max_frames)

    def set_ladder_mode(self, mode):
        pass

    def close(self):
        pass


def test_receiver_refusals(monkeypatch):
    monkeypatch.setattr(_lib, "Handle", NoDevice)
    kw = dict(autostart=False, sample_rate=48000, iq=True, dial_offsets_hz=(-1000.0, 2000.0))
    with pytest.raises(_lib.Ft8rxError, match="ft4_early_decode_s"):
        receiver.Receiver("", None, ft4_early_decode_s=(7.5,), **kw)
    with pytest.raises(_lib.Ft8rxError, match=r"modes: one per channel \(2\), got 1"):
        receiver.Receiver("", None, modes=("FT4",), **kw)
    with pytest.raises(_lib.Ft8rxError, match="modes: unknown mode"):
        receiver.Receiver("", None, modes=("FT8", "PSK31"), **kw)
    with pytest.raises(_lib.Ft8rxError, match="modes: .* wide live input"):
        receiver.Receiver("", None, autostart=False, modes="FT4")
    # each opt-in FT4 does not run with, by name, for an FT4 channel anywhere in the list ...
    for knobs, name in ((dict(my_call="K1ABC"), "my_call / dx_call"), (dict(dx_call="W9XYZ"), "my_call / dx_call"), (dict(recall=True), "recall"),
                        (dict(weak=True), "weak=True"), (dict(reports=True), "reports=True"), (dict(noise_blanker=True), "noise_blanker"),
                        (dict(float_frames=True), "float_frames")):
        for modes in ("FT4", ("FT8", "FT4")):
            with pytest.raises(_lib.Ft8rxError, match="FT4 decoding .* is not supported together with " + name.replace("/", ".")):
                receiver.Receiver("", None, modes=modes, **knobs, **kw)
        rx = receiver.Receiver("", None, autostart=False, **knobs)                      # ... at start() too, and no stream has opened
        with pytest.raises(_lib.Ft8rxError, match="is not supported together with"):
            rx._set_wide_in(48000, True, (-1000.0, 2000.0), None, None, False, False, ("FT4", "FT8"))
        assert rx.wide_in is None
        for modes in (None, "FT8", ("FT8", "FT8")):                                     # every channel FT8: what it always was
            assert receiver.Receiver("", None, **({} if modes is None else {"modes": modes}), **knobs, **kw).wide_in.modes is None
    rx = receiver.Receiver("", None, modes=("FT8", "FT4"), waterfall=True, bands=("20m", "20m"), **kw)
    assert rx.wide_in.modes == ("FT8", "FT4") and rx.ft4_early_samples == (72000,) and rx.wide_in.search_grid is not None
    with pytest.raises(_lib.Ft8rxError, match=r"search\(channel=1\): channel 1 is an FT4 channel"):
        rx._search_source(1)
    assert rx._search_source(0)[1] == "20m"
    assert receiver.Receiver("", None, modes="FT4", ft4_early_decode_s=(), **kw).ft4_early_samples == ()


# ---- 4. the ABI
def test_header_and_prototype_table():
    text = open(os.path.join(ROOT, "include", "ft8rx.h")).read()
    header = c_prototypes(text, r"ft8rx_ddc_stream_frames")
    assert list(header) == ["ft8rx_ddc_stream_frames"]
    assert mismatches({"ft8rx_ddc_stream_frames": _abi.PROTOTYPES["ft8rx_ddc_stream_frames"]}, header) == []
    assert len(_abi.PROTOTYPES["ft8rx_ddc_stream_frames"][1]) == 7
    assert text.count("ft8rx_ddc_stream_frames") >= 2                                   # the entry list and the declaration


def test_built_library_exports_the_symbol():
    for wide in (False, True):
        assert getattr(_lib.lib(wide), "ft8rx_ddc_stream_frames").argtypes == list(_abi.PROTOTYPES["ft8rx_ddc_stream_frames"][1])
    assert callable(_lib.Handle.ddc_stream_frames)


# ---- 5. the argument checks under the host sanitizers
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_frame_arguments_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ddc_frames_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "ddc_frames_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr
    assert "ddc frames arguments:" in p.stdout and int(p.stdout.split(":")[1].split()[0]) > 5000
