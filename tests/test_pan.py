"""The panorama on the CPU (no GPU needed): the float64 twin (pyft8_amd/pan.py) against a direct DFT matrix,
Parseval, the periodic Hann's leakage of bin-centred tones, the axes, the keyword's refusals, the stream twin against the whole stream
for every chunking, the host-only ABI entries, and the index arithmetic (csrc/pan_ring.hpp) under the host sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import pan_cases as cases
from conftest import ROOT
from pyft8_amd import _lib, pan
from pyft8_amd import kinds as K

IDS = [cases.KIND_IDS[k] for k in cases.KINDS]


@pytest.mark.parametrize("kind", cases.KINDS, ids=IDS)
def test_twin_is_the_direct_dft_at_256(kind):
    N, A = 256, 3
    x = cases.noisy(kind, cases.accuracy_n(N, A))
    rows, stats = pan.reference(x, kind, N, A)
    v = K.values(x, kind)
    w = pan.window(N).astype(np.float64)
    i = np.arange(N)
    F = np.exp(-2j * np.pi * np.outer(i, i) / N)
    want = np.zeros((2, N))
    for r in range(2):
        for a in range(A):
            X = F @ (w * v[(r * A + a) * N:(r * A + a + 1) * N])
            want[r] += np.abs(X) ** 2
    want = np.concatenate([want[:, N // 2:], want[:, :N // 2]], axis=1) if K.is_iq(kind) else want[:, :N // 2]
    assert rows.shape == want.shape == (2, pan.bins(kind, N))
    assert np.abs(rows - want).max() <= 1e-11 * want.max()
    assert (stats is None) == (not K.is_integer(kind))


def test_window_is_the_periodic_hann_and_the_library_table():
    L = _lib.lib()
    for N in (256, 512, 1024, 2048, 4096, 8192):
        w = pan.window(N)
        assert w.dtype == np.float32 and w[0] == 0.0 and w[N // 2] == 1.0 and np.array_equal(w[1:], w[1:][::-1])
        got = np.zeros(N, np.float32)
        assert L.ft8rx_pan_window(N, got.ctypes.data, N) == N and got.tobytes() == w.tobytes()
    assert L.ft8rx_pan_window(128, None, 0) == -1 and L.ft8rx_pan_window(3000, None, 0) == -1 and L.ft8rx_pan_window(2048, None, 0) == 2048


@pytest.mark.parametrize("kind", [K.IQ_I16, K.IQ_F32, K.WIDE_IQ_U8, K.WIDE_IQ_I8], ids=["iq_i16", "iq_f32", "iq_u8", "iq_i8"])
def test_parseval_for_iq(kind):
    N, A = 512, 4
    x = cases.noisy(kind, 2 * N * A)
    rows, _ = pan.reference(x, kind, N, A)
    wv = (K.values(x, kind).reshape(2, A, N) * pan.window(N).astype(np.float64)).reshape(2, -1)
    want = N * (np.abs(wv) ** 2).sum(axis=1)
    assert np.abs(rows.sum(axis=1) - want).max() <= 1e-12 * want.max()


@pytest.mark.parametrize("k0", [5, -5, 100, -127])
def test_bin_centred_iq_tone_peaks_where_it_should_with_hann_leakage(k0):
    """an exponential at bin k0 peaks at j = N / 2 + k0; the two neighbours hold exactly a quarter of the peak power and every other
    bin is at rounding: the periodic Hann window's three-point kernel (-1/4, 1/2, -1/4)"""
    N, A, kind = 256, 2, K.IQ_F32
    x = cases.store(cases.tone(kind, 2 * N, k0 / N, 1000.0), kind)
    rows, _ = pan.reference(x, kind, N, A)
    j0 = N // 2 + k0
    peak = A * (1000.0 * N / 2) ** 2
    for row in rows:
        assert int(np.argmax(row)) == j0 and abs(row[j0] - peak) <= 1e-6 * peak
        assert abs(row[j0 - 1] - peak / 4) <= 1e-6 * peak and abs(row[(j0 + 1) % N] - peak / 4) <= 1e-6 * peak
        others = np.delete(row, [j0 - 1, j0, (j0 + 1) % N])
        assert others.max() <= 1e-10 * peak
    assert np.allclose(pan.db(rows, kind, N, A)[:, j0], 20 * np.log10(1000.0 / 32768.0), atol=1e-4)


def test_real_sine_at_bin_k0():
    N, A, kind, k0 = 256, 1, K.REAL_F32, 40
    x = cases.store(cases.tone(kind, N, k0 / N, 32768.0), kind)
    rows, _ = pan.reference(x, kind, N, A)
    peak = (32768.0 * N / 4) ** 2
    assert rows.shape == (1, N // 2) and int(np.argmax(rows[0])) == k0 and abs(rows[0, k0] - peak) <= 1e-6 * peak
    assert abs(rows[0, k0 - 1] - peak / 4) <= 1e-6 * peak and abs(rows[0, k0 + 1] - peak / 4) <= 1e-6 * peak
    assert np.delete(rows[0], [k0 - 1, k0, k0 + 1]).max() <= 1e-10 * peak
    assert abs(pan.db(rows, kind, N, A)[0, k0]) <= 1e-4                 # a full-scale real sine is 0 dB


def test_uint8_constants_and_silence():
    """uint8 has no code that maps to zero: the constants 127 and 128 (-128 and +128 on the int16 scale) give a DC bin of (128 N / 2)^2
    per window with a quarter of it on either side; a silent int16 stream gives zero rows"""
    N, A = 256, 3
    for code in (127, 128):
        rows, stats = pan.reference(np.full((N * A, 2), code, np.uint8), K.WIDE_IQ_U8, N, A)
        dc = 2 * A * (128.0 * N / 2) ** 2                                # I and Q both; the weights are float32: 2^-24 each, twice that in power
        tol = 2.0 ** -22 * dc
        assert abs(rows[0, N // 2] - dc) <= tol and abs(rows[0, N // 2 - 1] - dc / 4) <= tol and abs(rows[0, N // 2 + 1] - dc / 4) <= tol
        assert np.array_equal(stats, [[0, 1]])
    rows, stats = pan.reference(np.zeros(N * A, np.int16), K.REAL_I16, N, A)
    assert not rows.any() and np.array_equal(stats, [[0, 0]])


def test_statistics_of_the_twin():
    N, A = 256, 2
    x = np.zeros((2 * N * A + 5, 2), np.int8)
    x[0, 0], x[N * A - 1, 1], x[N * A, 0], x[7, :] = -128, 127, 5, (127, -128)      # three samples at a rail in row 0, none in row 1
    x[2 * N * A, 0] = 127                                                           # behind the last complete row
    _, stats = pan.reference(x, K.WIDE_IQ_I8, N, A)
    assert np.array_equal(stats, [[3, 128], [0, 5]])
    u = np.full((N, 2), 128, np.uint8)
    u[3, 1], u[9, 0] = 0, 255
    assert np.array_equal(pan.reference(u, K.WIDE_IQ_U8, N, 1)[1], [[2, 255]])
    assert pan.reference(np.zeros(N, np.float32), K.REAL_F32, N, 1)[1] is None


def test_freqs_and_rows_done():
    f = pan.freqs(K.IQ_I16, 240000, 256)
    assert f.shape == (256,) and f[0] == -120000.0 and f[128] == 0.0 and f[129] == 937.5 and f[-1] == 120000.0 - 937.5
    f = pan.freqs(K.WIDE_REAL_I16, 64800000, 2048)
    assert f.shape == (1024,) and f[0] == 0.0 and f[1] == 64800000 / 2048 and f[-1] == 32400000 - 64800000 / 2048
    L = _lib.lib()
    out = (C.c_uint64 * 2)()
    for n_origin in (0, 1, 255, 256, 768, 769, (1 << 40) + 7):
        for n_end in [n_origin + d for d in (0, 1, 255, 256, 767, 768, 769, 5000)]:
            for N, A in ((256, 1), (256, 3), (512, 2)):
                assert L.ft8rx_pan_rows_done(n_origin, n_end, N, A, out) == 0
                assert (int(out[0]), int(out[1])) == pan.rows_done(n_origin, n_end, N, A), (n_origin, n_end, N, A)
                r_first, r_done = pan.rows_done(n_origin, n_end, N, A)
                assert r_first * A * N >= n_origin > (r_first - 1) * A * N and r_done >= r_first
                assert r_done == r_first or r_done * A * N <= n_end
                assert (r_done + 1) * A * N > n_end
    assert L.ft8rx_pan_rows_done(10, 5, 256, 1, out) == -1 and L.ft8rx_pan_rows_done(0, 5, 100, 1, out) == -1 and L.ft8rx_pan_rows_done(0, 5, 256, 0, out) == -1
    assert pan.held(0, 256 * 10, 256, 1, 4) == (6, 10) and pan.held(0, 256 * 3, 256, 1, 4) == (0, 3) and pan.held(300, 256 * 10, 256, 2, 256) == (1, 5)


def test_keyword_and_refusals():
    assert pan.params(None, 240000) is None and pan.params(False, 240000) is None
    assert pan.params(True, 240000) == (2048, 19, 256)                   # rint(0.16 * 240000 / 2048) = rint(18.75)
    assert pan.params(True, 64800000) == (2048, 5062, 256) and pan.params(True, 12000) == (2048, 1, 256)
    assert pan.params({"n_fft": 512, "n_avg": 7, "rows": 10}, 48000) == (512, 7, 10)
    assert pan.params({"period_s": 1.0, "n_fft": 256}, 48000) == (256, 188, 256)
    for bad, name in (({"n_fft": 128}, "n_fft"), ({"n_fft": 3000}, "n_fft"), ({"n_fft": 16384}, "n_fft"), ({"n_avg": 0}, "n_avg"), ({"n_avg": 65537}, "n_avg"),
                      ({"n_avg": 2.5}, "n_avg"), ({"rows": 0}, "rows"), ({"nfft": 256}, "nfft"), ({"period_s": 0}, "period_s"),
                      ({"n_avg": 3, "period_s": 1.0}, "both"), ("yes", "panorama"), (7, "panorama")):
        with pytest.raises(_lib.Ft8rxError, match=name):
            pan.params(bad, 240000)
    with pytest.raises(_lib.Ft8rxError, match="panorama: 2 streams"):
        pan.one_stream(True, 2)
    pan.one_stream(None, 2)
    pan.one_stream(True, 1)
    with pytest.raises(_lib.Ft8rxError, match="kind"):
        pan.reference(np.zeros(256, np.int16), 7, 256, 1)
    with pytest.raises(_lib.Ft8rxError, match="ONE stream"):
        pan.pack(np.zeros((2, 256), np.int16), K.REAL_I16)


@pytest.mark.parametrize("n_origin", [0, 3 * 256 + 17, (1 << 40) + 255])
@pytest.mark.parametrize("kind", [K.WIDE_IQ_U8, K.REAL_I16, K.IQ_F32], ids=["iq_u8", "real_i16", "iq_f32"])
def test_stream_twin_equals_the_whole_stream_for_every_chunking(kind, n_origin):
    N, A = 256, 3
    x = cases.noisy(kind, 7 * N * A + 111)
    rows, stats = pan.reference(x, kind, N, A, n_origin=n_origin)
    r_first, r_done = pan.rows_done(n_origin, n_origin + len(x), N, A)
    assert len(rows) == r_done - r_first >= 6
    for name, lengths in cases.chunkings(len(x), N, A, len(x)).items():
        out = pan.reference_stream(cases.cut(x, lengths), kind, N, A, n_origin=n_origin)
        at = r_first
        for r0, rr, ss in out:
            assert r0 == at, name
            at += len(rr)
        assert at == r_done
        got = np.concatenate([rr for _, rr, _ in out])
        assert got.tobytes() == rows.tobytes(), name
        if stats is not None:
            assert np.array_equal(np.concatenate([ss for _, _, ss in out]), stats), name


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_ring_arithmetic_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "pan_ring_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "pan_ring_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr
    assert "pan ring arithmetic:" in p.stdout and int(p.stdout.split(":")[1].split()[0]) > 100000
