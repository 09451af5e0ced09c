"""The spectrogram stage behind the streaming down-converter, without a GPU: its index arithmetic under the host
sanitizers (tests/ddc_grid_ring_check.cpp), the pure Python mapping of device rows to cycles, hops and grid rows against a brute-force
model, the declarations of the three entry points, and the opt-in's off state (tests/test_gpu_ddc_grid.py holds the kernel to
k_spectrogram on the GPU)."""
import inspect
import os
import re
import shutil
import subprocess
import threading

import numpy as np
import pytest

from conftest import ROOT
from pyft8_amd import _abi, _lib, wide_in
from pyft8_amd.receiver import Receiver

NSAMP, HOP, TILE = 180000, 480, 1008
ENTRIES = ("ft8rx_ddc_stream_grid_open", "ft8rx_ddc_stream_grid_info", "ft8rx_ddc_stream_grid_read")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_grid_ring_arithmetic_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ddc_grid_ring_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "ddc_grid_ring_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr
    assert "ddc grid ring arithmetic:" in p.stdout and int(p.stdout.split(":")[1].split()[0]) > 100000


# ---- the mapping: device row q <-> (cycle, hop) -> row of the 750-row grid
def brute_rows(t_first, m_end):
    """{q: (cycle, hop, grid row)} for every row that exists when the outputs [0, m_end) do, from the definitions alone: the first
    cycle the scheduler decodes starts at m_c0 (at least -6000), cycle c0 + i starts 180000 i later, hop h of a cycle ends at
    m_c + 480 h, row q ends at p0 + 480 q, and a row exists iff it ends inside (0, m_end]"""
    c0 = int(t_first // 15) - 1
    while int(round((15 * c0 - t_first) * 12000)) < -6000:
        c0 += 1
    m_c0 = int(round((15 * c0 - t_first) * 12000))
    p0 = m_c0 % HOP
    ends = {p0 + HOP * q: q for q in range(0, m_end // HOP + 2) if 0 < p0 + HOP * q <= m_end}
    out = {}
    for i in range(-1, m_end // NSAMP + 2):
        for h in range(1, 376):
            e = m_c0 + NSAMP * i + HOP * h
            if e in ends:
                assert ends[e] not in out
                out[ends[e]] = (c0 + i, h, (375 * ((c0 + i) % 2) + h) % 750)
    assert len(out) == len(ends)                                                       # every row is exactly one hop of one cycle
    return c0, m_c0, p0, out


@pytest.mark.parametrize("t_first,p0,m_c0", [(15000.0, 0, 0), (15014.2, 0, 9600), (15015.0 - 1 / 12000, 1, 1), (15015.0 - 479 / 12000, 479, 479),
                                             (15000.0 + 343 / 12000, 137, -343), (15000.4, 0, -4800), (30.0 + 1 / 12000, 479, -1)])
def test_rows_cycles_and_grid_rows(t_first, p0, m_c0):
    """p0 in {0, 1, 137, 479}, first cycles that start before the stream (negative m_c), an odd first cycle: place / row_of / phase
    against the brute-force model over 2.2 cycles, and the rows a push completes against it for irregular advances of m_produced"""
    m_end = 2 * NSAMP + 40000
    c0, mc, p, want = brute_rows(t_first, m_end)
    s = wide_in.PassScheduler(t_first, ())
    assert (s.cycle, s.cycle_start(s.cycle)) == (c0, mc) and (mc, p) == (m_c0, p0)
    assert wide_in.grid_phase(mc) == p0 and 0 <= p0 < HOP
    for q, (c, h, r) in want.items():
        assert wide_in.grid_place(q, mc, c0) == (c, h, r) and wide_in.grid_row_of(c, h, mc, c0) == q
    # hop h of every cycle the scheduler decodes ends where the frame's hop h does: m_c + 480 h
    for c in (c0, c0 + 1):
        for h in (1, 8, 375):
            assert p0 + HOP * wide_in.grid_row_of(c, h, mc, c0) == s.cycle_start(c0) + NSAMP * (c - c0) + HOP * h
    # the odd cycle's hop 375 wraps to grid row 0, the even cycle's hop 1 is row 1, the odd cycle's hop 1 row 376
    odd = c0 if c0 % 2 else c0 + 1
    assert wide_in.grid_place(wide_in.grid_row_of(odd, 375, mc, c0), mc, c0) == (odd, 375, 0)
    assert wide_in.grid_place(wide_in.grid_row_of(odd, 1, mc, c0), mc, c0)[2] == 376
    assert wide_in.grid_place(wide_in.grid_row_of(odd + 1, 1, mc, c0), mc, c0)[2] == 1
    # pushes: m_produced advances in whole tiles, 0 .. 12 at a time; the rows completed are the model's, each exactly once
    m, seen, seed = 0, [], 12345
    while m < m_end - 13 * TILE:
        seed = (seed * 1664525 + 1013904223) % 2 ** 32
        m_new = m + TILE * ((seed >> 24) % 13)
        a, b = wide_in.grid_rows_completed(m, m_new, p0)
        assert list(range(a, b)) == sorted(q for q in want if m < p0 + HOP * q <= m_new)
        assert b == wide_in.grid_hops_done(m_new, p0)
        seen += range(a, b)
        m = m_new
    assert seen == sorted(q for q in want if p0 + HOP * q <= m) and len(seen) > 750
    # more new rows than the ring holds: the newest n_rows
    assert wide_in.grid_rows_completed(0, 12096, 0, 16) == (10, 26) and wide_in.grid_rows_completed(0, 0, p0) == (wide_in.grid_hops_done(0, p0),) * 2


# ---- the declarations
def test_entry_points_are_declared():
    hdr = open(os.path.join(ROOT, "include", "ft8rx.h")).read()
    for name in ENTRIES:
        assert name in _abi.PROTOTYPES
        assert re.search(r"^int\s+" + name + r"\(ft8rx_handle\* h,", hdr, re.M), name
    for name in ("ddc_stream_grid_open", "ddc_stream_grid_info", "ddc_stream_grid_read"):
        assert callable(getattr(_lib.Handle, name))
    hpp = open(os.path.join(ROOT, "pyft8_amd", "csrc", "ddc_grid_ring.hpp")).read()
    assert "hip" not in hpp.replace("No HIP", "").lower()                              # pure index arithmetic


# ---- the live layer without a GPU: what WideIn asks of the handle, from the arithmetic alone
class FakeHandle:
    grid_cols = 976

    def __init__(self, D, n_out):
        self.D, self.n, self.n_out, self.grid, self.reads = D, 0, n_out, None, []

    def ddc_stream_open(self, kind, rate, n_streams, src, dials):
        return np.zeros(len(src))

    def ddc_stream_push(self, a):
        self.n += a.shape[1]
        return wide_in.produced(self.n, self.D)


class FakeGridHandle(FakeHandle):
    def ddc_stream_grid_open(self, hop_phase, n_rows):
        assert self.n == 0 and self.grid is None
        self.grid = (hop_phase, n_rows)

    def ddc_stream_grid_read(self, q_first, n):
        p0, n_rows = self.grid
        q_next = wide_in.grid_hops_done(wide_in.produced(self.n, self.D), p0)
        assert n >= 1 and q_first + n <= q_next and q_first >= q_next - n_rows                # what the library would refuse
        self.reads += range(q_first, q_first + n)
        # row q of channel j holds q + j / 4 in every column
        return (np.arange(q_first, q_first + n, dtype=np.float32)[None, :, None] + np.arange(self.n_out, dtype=np.float32)[:, None, None] / 4
                + np.zeros((1, 1, self.grid_cols), np.float32))


class FakeAudioIn:
    df = 3.125

    def __init__(self):
        self.search_grid = np.ones((750, 976), np.float32)
        self.waterfall_data = {"data": self.search_grid[::2, ::2].T, "df": 6.25, "dt": 0.08, "sig_w": 158, "sig_h": 8, "pixels_per_cycle": 187}


class FakeReceiver:
    def __init__(self, handle, t):
        self.h, self._live_lock, self._stop = handle, threading.RLock(), threading.Event()
        self.early_decode_hops, self.thread_error, self.audio_in = (), None, FakeAudioIn()
        self.time_source = lambda: t

    def _live_handle(self, n_frames=1):
        return self.h


def test_off_builds_no_grid_and_on_fills_it():
    D, rate, t_first = 2, 24000, 15000.0 + 343 / 12000
    x = np.ones((rate * 17, 2), np.int16)
    # off (the default): no grid, no waterfall, and none of the grid calls (FakeHandle has none of them)
    rx = FakeReceiver(FakeHandle(D, 2), t_first)
    w = wide_in.WideIn(rx, rate, iq=True, dial_offsets_hz=(-1000.0, 2000.0))
    w.push(x)
    assert w.waterfall is False and w.search_grid is None and w.waterfall_data is None and w.grid_phase is None
    assert inspect.signature(Receiver.__init__).parameters["waterfall"].default is False
    assert inspect.signature(Receiver.start).parameters["waterfall"].default is False
    assert inspect.signature(Receiver.search).parameters["channel"].default is None
    # on: every row read exactly once, in order, and written at its place
    rx = FakeReceiver(FakeGridHandle(D, 2), t_first)
    w = wide_in.WideIn(rx, rate, iq=True, dial_offsets_hz=(-1000.0, 2000.0), bands=("20m", "17m"), waterfall=True)
    assert [g.shape for g in w.search_grid] == [(750, 976)] * 2 and all((g == 1.0).all() for g in w.search_grid)
    cuts = [0, 1, 4801, 4801 + rate, 9 * rate + 7, 17 * rate]
    for a, b in zip(cuts, cuts[1:]):
        w.push(x[a:b])
    w.flush()
    assert rx.h.grid == (137, 750) and w.grid_phase == 137
    q_next = wide_in.grid_hops_done(w.m_produced, 137)
    assert rx.h.reads == list(range(0, q_next)) and q_next > 375 + 40
    c0, m_c0 = 1000, -343
    for j, g in enumerate(w.search_grid):
        for q in range(q_next):
            c, h, r = wide_in.grid_place(q, m_c0, c0)
            assert (g[r] == np.float32(q + j / 4)).all(), (j, q)
        untouched = sorted(set(range(750)) - {wide_in.grid_place(q, m_c0, c0)[2] for q in range(q_next)})
        assert untouched and (g[untouched] == 1.0).all()
        assert set(w.waterfall_data[j]) == set(rx.audio_in.waterfall_data)
        assert np.shares_memory(w.waterfall_data[j]["data"], g) and w.waterfall_data[j]["data"].shape == rx.audio_in.waterfall_data["data"].shape
    assert w.grid_cycle(0) == 1000 and w.grid_cycle(1) is None


def test_search_refuses_a_channel_without_a_grid():
    """Receiver.search(channel=) names what is missing: no wide input, a wide input without waterfall=True, a channel out of range"""
    rx = Receiver.__new__(Receiver)                          # (constructing a Receiver needs a GPU; the refusals do not)
    rx.band, rx.audio_in, rx.wide_in = None, FakeAudioIn(), None
    with pytest.raises(_lib.Ft8rxError, match=r"search\(channel=0\).*waterfall=True"):
        rx.search("x", 0, channel=0)
    fake = FakeReceiver(FakeGridHandle(2, 2), 15000.0)
    rx.wide_in = wide_in.WideIn(fake, 24000, iq=True, dial_offsets_hz=(-1000.0, 2000.0))
    with pytest.raises(_lib.Ft8rxError, match=r"search\(channel=1\).*waterfall=True"):
        rx.search("x", 0, channel=1)
    rx.wide_in = wide_in.WideIn(fake, 24000, iq=True, dial_offsets_hz=(-1000.0, 2000.0), bands=("20m", "17m"), waterfall=True)
    for bad in (2, -1):
        with pytest.raises(_lib.Ft8rxError, match=r"channels 0 \.\. 1"):
            rx.search("x", 0, channel=bad)
    assert rx._search_source(1)[1] == "17m" and rx._search_source(1)[0] is rx.wide_in.search_grid[1]
    assert rx._search_source(None) == (rx.audio_in.search_grid, None)
