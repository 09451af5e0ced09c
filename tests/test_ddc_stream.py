"""The streaming down-converter and the wide live input on the CPU (no GPU needed): the continuous float64 twin
(pyft8_amd/ddc.py: reference_stream) against the one-shot twin, the pass scheduler of the live layer (pyft8_amd/wide_in.py), the inputs of
the live end-to-end test against the CPU oracle, and the ring arithmetic (csrc/ddc_ring.hpp) under the host sanitizers."""
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

import ddc_cases as cases
import ddc_stream_cases as live
from conftest import ROOT
from pyft8_amd import ddc, wide_in

NSAMP = 180000
TILE = 1008


# ---- 1. the twin
@pytest.mark.parametrize("D,kind", [(1, ddc.IQ_I16), (2, ddc.IQ_I16), (4, ddc.IQ_I16), (4, ddc.REAL_I16), (16, ddc.IQ_I16)])
def test_reference_stream_is_reference(D, kind):
    """n_origin = 0 and the outputs [0, 180000) of a 15-s input: the same float64 sums (1e-9 counts covers FFT against direct
    convolution).  The input is that of tests/test_ddc.py's two-channel test."""
    iq, offs, _ = cases.recipe(0, D, only_a=(D == 1))
    x = iq if ddc.is_iq(kind) else iq[:, 0]
    f = offs[0] if ddc.is_iq(kind) else 0.25 * 12000 * D
    y, _ = ddc.reference(x, kind, 12000 * D, f, gain=1.5)
    ys = ddc.reference_stream(x, kind, 12000 * D, f, 0, NSAMP, gain=1.5)
    assert ys.dtype == np.float64 and ys.shape == (NSAMP,) and np.abs(y).max() > 1000
    assert np.abs(ys - y).max() <= 1e-9
    # any range, before the origin too (where the input is zero), is the same stream
    part = ddc.reference_stream(x, kind, 12000 * D, f, -300, 2001, gain=1.5)
    assert np.abs(part[300:] - y[:2001]).max() <= 1e-9 and np.abs(part[:150]).max() <= 1e-9


def test_reference_stream_takes_any_length_and_origin():
    """More than 15 s is one stream: outputs across 180000 equal those of the same samples fed as a stream that begins later"""
    rng = np.random.Generator(np.random.Philox(key=0x16))
    x = rng.integers(-32768, 32768, size=(24000 * 16, 2)).astype(np.int16)
    y = ddc.reference_stream(x, ddc.IQ_I16, 24000, 1234.5, NSAMP - 500, NSAMP + 500)
    cut = 2 * (NSAMP - 3000)
    y2 = ddc.reference_stream(x[cut:], ddc.IQ_I16, 24000, 1234.5, NSAMP - 500, NSAMP + 500, n_origin=cut)
    assert np.abs(y).max() > 1000 and np.abs(y - y2).max() <= 1e-9          # (the 3000 outputs dropped lie beyond the filters' reach)
    with pytest.raises(ddc._lib.Ft8rxError, match="rate"):
        ddc.reference_stream(x, ddc.IQ_I16, 44100, 0.0, 0, 10)
    with pytest.raises(ddc._lib.Ft8rxError, match="m_lo"):
        ddc.reference_stream(x, ddc.IQ_I16, 24000, 0.0, 10, 10)


@pytest.mark.parametrize("k", [5, 1065220])
def test_origin_shift_and_the_phase_rule(k):
    """The same samples as a stream that begins s = k 1008 D later, asked for the outputs shifted by s / D.  The phase rule: the mixer
    of the shifted stream is ahead by phi = (w s mod 2^32) / 2^32 cycles, u'[n + s] = u[n] e^{-2 pi i phi}, and i^m is unchanged because
    s / D = 1008 k is a multiple of 4.  So the shifted stream of x e^{+2 pi i phi} gives the values of x -- and where w s = 0 (mod 2^32)
    the shifted stream of x itself does.  k = 1065220 puts the shifted stream across n = 2^32."""
    D, rate = 4, 48000
    iq, offs, _ = cases.recipe(0, D)
    x = iq[:rate].astype(np.float64)
    x = x[:, 0] + 1j * x[:, 1]
    s = k * TILE * D
    assert k == 5 or s < 2 ** 32 < s + len(x)
    lo, hi = -100, 11000
    for f in (offs[0], 6000.0):
        w, _ = ddc.frequency_word(rate, f)
        y = ddc.reference_stream(x, ddc.IQ_F32, rate, f, lo, hi)
        phi = ((w * s) % 2 ** 32) / 2.0 ** 32
        assert (f == 6000.0) == (phi == 0.0)
        ys = ddc.reference_stream(x * np.exp(2j * np.pi * phi), ddc.IQ_F32, rate, f, lo + s // D, hi + s // D, n_origin=s)
        assert np.abs(y).max() > 1000 and np.abs(ys - y).max() <= 1e-9
        if phi:                                                                       # without the rotation it is another signal
            assert np.abs(ddc.reference_stream(x, ddc.IQ_F32, rate, f, lo + s // D, hi + s // D, n_origin=s) - y).max() > 100


# ---- 2. the scheduler
def expected_passes(t_first, hops, m_end):
    """From the timing rule alone: cycle c starts at m_c = round((15 c - t_first) 12000) and is decoded if m_c >= -6000; its passes are
    the early hops (480 hop outputs) and the complete cycle (180000), each due once m_c + n_have outputs exist"""
    out = []
    c = int(t_first // 15) - 1
    while True:
        m_c = int(round((15 * c - t_first) * 12000))
        if m_c >= -6000:
            for hop, n_have in [(h, 480 * h) for h in hops] + [(0, NSAMP)]:
                if m_c + n_have > m_end:
                    return out
                out.append((c, hop, m_c, n_have))
        c += 1


@pytest.mark.parametrize("t_first,first_cycle,m_first", [(15014.2, 1001, 9600), (15000.4, 1000, -4800), (15000.5, 1000, -6000),
                                                          (15000.6, 1001, 172800), (15000.0, 1000, 0), (7.25, 1, 93000)])
def test_scheduler(t_first, first_cycle, m_first):
    """A 35-s stream at 48 kHz in irregular chunks: every pass comes due exactly once, in order, at the first chunk after which the
    outputs it needs exist (produced(): whole tiles), for a first sample in mid-cycle and on both sides of the 0.5-s rule"""
    D, rate, hops = 4, 48000, (320, 340)
    s = wide_in.PassScheduler(t_first, hops)
    assert (s.cycle, s.cycle_start(s.cycle)) == (first_cycle, m_first)
    total, n, got, lens, i = 35 * rate, 0, [], (1920, 1000, 47999, 13, 48000, 1), 0
    while n < total:
        before = wide_in.produced(n, D)
        n = min(total, n + lens[i % len(lens)])
        i += 1
        now = wide_in.produced(n, D)
        assert now % TILE == 0 and before <= now <= n // D and n // D - now <= 2 * TILE + 80          # a tile and the filters' reach
        for p in s.due(now):
            assert before < p[2] + p[3] <= now
            got.append(p)
    assert s.due(wide_in.produced(n, D)) == []
    want = expected_passes(t_first, hops, wide_in.produced(total, D))
    assert got == want and len(want) >= 3 and want[0][0] == first_cycle and want[0][2] == m_first
    if t_first == 15014.2:
        assert want == [(1001, 320, 9600, 153600), (1001, 340, 9600, 163200), (1001, 0, 9600, NSAMP),
                        (1002, 320, 189600, 153600), (1002, 340, 189600, 163200), (1002, 0, 189600, NSAMP)]
    assert wide_in.PassScheduler(t_first, ()).due(10 ** 6)[0] == (first_cycle, 0, m_first, NSAMP)          # no early hops: whole cycles


class FakeHandle:
    """What WideIn asks of the live handle, from the ring arithmetic alone"""
    def __init__(self, D):
        self.D, self.n, self.chunks = D, 0, []

    def ddc_stream_open(self, kind, rate, n_streams, src, dials):
        self.opened = (kind, rate, n_streams, list(src), list(dials))
        return np.zeros(len(src))

    def ddc_stream_push(self, a):
        assert 1 <= a.shape[1] <= 12000 * self.D
        self.n += a.shape[1]
        self.chunks.append((a.shape[1], bool(a.any())))
        return wide_in.produced(self.n, self.D)


class FakeReceiver:
    def __init__(self, D):
        self.h, self._live_lock, self._stop = FakeHandle(D), threading.RLock(), threading.Event()
        self.early_decode_hops, self.thread_error = (320,), None
        self.time_source = lambda: 15000.0

    def _live_handle(self, n_frames=1):
        return self.h


@pytest.mark.parametrize("n_real,due", [(153600 * 4, True), (153600 * 4 - 3, True), (153600 * 4 - 4, False)])
def test_end_of_source_flush(n_real, due):
    """A finite source ends 0 .. 4 samples short of hop 320 of its first cycle: the outputs of its last real sample exist only after
    the zeros of flush(), and the early pass is due iff those outputs reach 480 x 320"""
    D, rate = 4, 48000
    rx = FakeReceiver(D)
    w = wide_in.WideIn(rx, rate, iq=True, dial_offsets_hz=(-1000.0, 2000.0), bands=("a", "b"))
    x = np.ones((n_real, 2), np.int16)
    w.push(x[:100000])                                                                # longer than a second: handed on in seconds
    w.push(x[100000:])
    assert rx.h.opened == (ddc.IQ_I16, rate, 1, [0, 0], [-1000.0, 2000.0]) and w.t_first == 15000.0
    assert [c[0] for c in rx.h.chunks[:3]] == [48000, 48000, 4000] and all(c[1] for c in rx.h.chunks)
    assert w.n_pushed == n_real and w.m_produced < 153600 and w._ready == []
    w.flush()
    assert all(not c[1] for c in rx.h.chunks if c[0] == TILE * D) and rx.h.chunks[-1] == (TILE * D, False)
    assert w.m_produced >= -(-n_real // D) and w.n_pushed == n_real
    assert w._ready == ([(1000, 320, 0, 153600)] if due else [])
    # the same through the feeder thread of open()
    rx2 = FakeReceiver(D)
    w2 = wide_in.WideIn(rx2, rate, iq=True, dial_offsets_hz=(-1000.0, 2000.0)).open(iter([x[:1920], x[1920:2920], x[2920:]]))
    w2.close(30.0)
    assert w2.source_exhausted and rx2.thread_error is None and w2._ready == w._ready and rx2.h.n == rx.h.n


# ---- 3. the inputs of the live test (tests/test_gpu_ddc_stream.py: test_live_end_to_end)
@pytest.mark.parametrize("i", live.USED)
def test_live_inputs(i):
    """The oracle decodes exactly the six transmitted texts from frame i, and from the frame with its analytic signal rotated by 1.0,
    2.5 and 4.0 rad (what a later cycle of a continuous mixer delivers).  (i = 0 does not qualify: CQ XN4EWX LK72 is in the difference.)"""
    want, words = live.messages(i)
    assert len(want) == 6 and len(words) == 6
    assert cases.oracle_texts(live.frame(i)) == want
    for phi in (1.0, 2.5, 4.0):
        assert cases.oracle_texts(live.rotated(live.frame(i), phi)) == want, phi


def test_live_stream_through_the_twin():
    """The control on the frames the live test uses: the twin's output for each channel and cycle of the two-cycle stream decodes to
    the six texts of the frame placed there"""
    x = live.stream()
    assert x.shape == (2 * NSAMP * 4, 2) and x.dtype == np.int16 and np.abs(x.astype(np.int32)).max() < 32767
    for c in range(2):
        for j in range(2):
            assert cases.oracle_texts(live.twin_frame(c, j)) == live.messages(live.PLAN[c][j])[0], (c, j)


# ---- the ring arithmetic under the host sanitizers
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_ring_arithmetic_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ddc_ring_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "ddc_ring_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr
    assert "ddc ring arithmetic:" in p.stdout and int(p.stdout.split(":")[1].split()[0]) > 100000
    # the Python twin of the tile count (wide_in.produced) is the header's
    for D in (1, 2, 4, 8, 16):
        r2 = 1 if D == 1 else 2
        assert wide_in._last_input(D) == ((TILE - 1) * r2 + (len(ddc.taps(12000 * D, 2)) - 1) // 2) * (D // r2) + max(0, (len(ddc.taps(12000 * D, 1)) - 1) // 2)
