"""The FT4 weak search without a GPU: the twin pyft8_amd/ft4.py weak_sums / weak_grid / weak_score_map /
search_weak -- its sums against the coherent step's, the FFT form against the direct sums, designed signals, the edges, the gain on
fixed seeds, the margins of the GPU test's fixtures -- then which calls Receiver(ft4_weak=True) makes on its handle, and the new entry
points in the header, the prototype table and the built library."""
import os
import types

import numpy as np
import pytest

import ft4_cases as cases
import ft4_weak_cases as wc
from conftest import ROOT
from pyft8_amd import _abi, _lib, ft4, receiver
from test_abi import c_prototypes, mismatches

NEW = ("ft8rx_ft4_set_weak", "ft8rx_ft4_weak_info", "ft8rx_ft4_sync_weak")
F0, H0 = cases.F0_RANGE, cases.H0_RANGE


# ---- 1. the twin
def test_sums_against_complex_amplitudes():
    """W[h0 + 4 s][4 f0][t] is C[s][t] of the coherent step at tt = ft = 0 up to one unit-modulus constant per candidate"""
    audio, cands = cases.demod_frames()
    for f, f0, h0, what in cands:
        C = ft4.complex_amplitudes(audio[f], f0, h0, 0, 0)
        W = ft4.weak_sums(audio[f], h0 + 4 * np.arange(ft4.NSYM), [4 * f0])[:, 0, :]
        top = np.abs(C).max()
        if top == 0.0:
            assert what == "all-zero frame" and not W.any()
            continue
        k = np.unravel_index(np.abs(C).argmax(), C.shape)
        u = W[k] / C[k]
        assert abs(abs(u) - 1.0) <= 1e-9, what
        assert np.abs(W - u * C).max() <= 1e-9 * top, what


def test_fft_form_is_the_direct_sums():
    x = cases.six()[0]
    lo, hi = H0[0] + 4, H0[1] + 4 * (ft4.NSYM - 2)
    G = ft4.weak_grid(x, lo, hi)
    assert G.shape == (hi - lo, ft4.WEAK_NFQ) and ft4.WEAK_NFQ == 2306           # 4 x 570 + 1 + 24: the top bin's highest tone
    rows = [lo, -4, -3, -1, 0, 1, 37, 300, 579, hi - 1]                          # before the frame, across its start, inside, the last one
    fqs = np.array([0, 1, 5, 7, 8, 9, 100, 1001, 1150, 2279, 2280, 2281])
    W = ft4.weak_sums(x, rows, fqs)
    top = np.abs(W).max()
    for i, r in enumerate(rows):
        for t in range(4):
            assert np.abs(W[i, :, t] - G[r - lo, fqs + 8 * t] * 1j ** ((t * r) % 4)).max() <= 1e-9 * top, (r, t)
    assert not G[:-4 - lo + 1].any() and G[-3 - lo].any()                       # rows up to -4 hold no sample of the frame


@pytest.mark.parametrize("q", [-2, -1, 0, 1])
def test_designed_signal_on_the_grid(q):
    """a noise-free signal at carrier 4 f0 + q that starts on a row: best[f0] within 2 % of 32, at that row, and the one candidate"""
    f0, h = 96, 40
    x = ft4.frame_with_signals(1, [(cases.DEMOD_WORD, (4 * f0 + q) * ft4.DF_HZ, ft4.HOP * h / ft4.FS, 0.0)], noise=False)
    out, best, bh, S, fq_lo = ft4.search_weak(x, *F0, *H0, full=True)
    assert [(c[0], c[1]) for c in out] == [(f0, h)] and abs(out[0][2] - 32.0) <= 0.02 * 32.0
    assert np.unravel_index(S.argmax(), S.shape) == (4 * f0 + q - fq_lo, h - H0[0])      # the map's peak is the signal's own carrier
    assert S.min() >= 0.0 and S.max() <= 32.0


def test_designed_signal_off_the_grid_and_the_edges():
    f0, h = 96, 40
    x = ft4.frame_with_signals(1, [(cases.DEMOD_WORD, (4 * f0 + 0.5) * ft4.DF_HZ, ft4.HOP * h / ft4.FS, 0.0)], noise=False)
    out = ft4.search_weak(x, *F0, *H0)
    assert [(c[0], c[1]) for c in out] == [(f0, h)] and out[0][2] > 27.0           # 1.3 Hz off: the right bin still
    row = lambda t: int(np.rint(t * ft4.FS / ft4.HOP))
    x = ft4.frame_with_signals(1, [(cases.DEMOD_WORD, 1000.0, -0.3, 0.0)], noise=False)
    out = ft4.search_weak(x, *F0, *H0)
    assert [(c[0], c[1]) for c in out] == [(96, row(-0.3))] and out[0][2] > 24.0   # the ramp and part of block a lie before the frame
    x = ft4.frame_with_signals(1, [(cases.DEMOD_WORD, 1500.0, 2.6, 0.0)], noise=False)
    out = ft4.search_weak(x, *F0, *wc.H0_WIDE)
    assert [(c[0], c[1]) for c in out] == [(144, row(2.6))] and out[0][2] > 22.0   # it runs past sample 89 999: block d is cut
    out, best, bh, S, _ = ft4.search_weak(cases.zero_frame(), *F0, *H0, full=True)
    assert out == [] and not S.any() and not best.any() and (bh == H0[0]).all()    # digital silence: score 0 everywhere, no candidate
    assert ft4.weak_best(np.zeros((2, 3)), 0, 0, 1, -42)[1][0] == -42               # f0 = 0: carriers -2 and -1 are not evaluated


@pytest.fixture(scope="module")
def gain():
    """The issue's recipe: range 12.5 .. 3000 Hz, frames 7000 .. 7003 of ten signals, noise frames 9100 .. 9105; both searches cut at
    the threshold that leaves `per` noise candidates per noise frame; a truth is found with a candidate within 1 bin and 2.5 rows
    -> {(snr, per): (found by the existing search, by the weak search)} of 40"""
    f0r, h0r = ft4.freq_range_to_f0((12.5, 3000.0)), H0

    def bests(x):
        o = ft4.search(ft4.grid_db(ft4.grid_power(x)), *f0r, *h0r, full=True)
        w = ft4.search_weak(x, *f0r, *h0r, full=True)
        return (o[1], o[2]), (w[1], w[2])

    kept = lambda b, thr: ft4._keep(b[0], b[1], f0r[0], thr, 10 ** 6)
    noise = [bests(ft4.make_frame(9100 + i, n_signals=0)) for i in range(6)]

    def threshold(k, per):
        sc = sorted((c[2] for n in noise for c in kept(n[k], -1e9)), reverse=True)
        return 0.5 * (sc[6 * per - 1] + sc[6 * per])

    out = {}
    for snr, per in ((-17, 1), (-15, 3)):
        thr, tot = [threshold(k, per) for k in (0, 1)], [0, 0]
        for i in range(4):
            x, truth = ft4.make_frame(7000 + i, n_signals=10, snr_range=(snr, snr), return_truth=True)
            b = bests(x)
            for k in (0, 1):
                cands = kept(b[k], thr[k])
                tot[k] += sum(any(abs(c[0] - t["f0"] / ft4.BIN_HZ) <= 1 and abs(c[1] - t["t0"] * ft4.FS / ft4.HOP) <= 2.5 for c in cands) for t in truth)
        out[(snr, per)] = (tot[0], tot[1], thr)
    return out


def test_gain_on_fixed_seeds(gain):
    for (snr, per), (old, new, thr) in gain.items():
        print(f"ft4 weak twin at {snr} dB, {per} noise candidate(s) per frame (thresholds {thr[0]:.2f} / {thr[1]:.3f}): {old} / {new} of 40 truths found")
    assert gain[(-17, 1)][0] <= 26 and gain[(-17, 1)][1] >= 32                     # measured 22 and 35
    assert gain[(-15, 3)][1] == 40


def test_the_gpu_fixtures_are_far_from_ties():
    """What tests/test_gpu_ft4_weak.py relies on, on the twin alone.  Lists: every decision behind them (threshold, neighbours, order,
    cut) lies further from a tie than twice the two scores' bounds together.  best_h0: the bin's winning h beats every other h of its block
    by more than twice the bound in all but a few bins per frame (measured: 2 of 565 on the six-signal frame, 3 on the noise frame, 1 on
    the edge frame); those few are the only ones the GPU test leaves out, so their share is pinned here."""
    for name in wc.FRAMES:
        t = wc.twin(name)
        m = min(wc.list_margin(t, wc.STAGE_WEAK_MIN, mc) for mc in (4, 256))
        clear = wc.h0_clear(t)
        print(f"ft4 weak fixture {name}: bound {wc.best_bound(t).max():.2e}, list margin {m:.1f} x, h0 clear in {int(clear.sum())} of {len(clear)} bins, "
              f"{len(wc.twin_list(t, F0[0], wc.STAGE_WEAK_MIN, 256))} candidates")
        assert m >= 2.0, name
        if name == "all zero":
            assert not t["best"].any() and not t["bound"].any()                 # exact zeros: compared exactly, no margin needed
        else:
            assert np.isfinite(t["bound"]).all() and t["bound"].max() <= 2e-3 and (~clear).sum() <= 3, name
    six, edges = wc.twin("six signals"), wc.twin("edges")
    assert len(wc.twin_list(six, F0[0], wc.STAGE_WEAK_MIN, 256)) >= 6 and len(wc.twin_list(wc.twin("noise"), F0[0], wc.STAGE_WEAK_MIN, 256)) > 4
    got = {c[0]: c[1] for c in wc.twin_list(edges, F0[0], wc.STAGE_WEAK_MIN, 256)}
    row = lambda s: int(np.rint(s * ft4.FS / ft4.HOP))
    assert got[F0[0]] == row(0.7) and got[F0[1] - 1] == row(1.1) and got[96] == row(-0.3) and got[144] == row(2.6)      # both ends of the range, both edges
    for rng in wc.narrow_ranges():
        t = wc.twin("six signals", *rng)
        assert wc.list_margin(t, wc.STAGE_WEAK_MIN, 256) >= 2.0 and wc.h0_clear(t).all(), rng
        assert [c[:2] for c in wc.twin_list(t, rng[0], wc.STAGE_WEAK_MIN, 256)] == [wc.strongest()[:2]], rng


def test_decode_twin_takes_the_weak_search():
    x, truth = cases.six()
    f0, h0 = wc.strongest()[:2]
    got = ft4.decode_twin(x, f0, f0 + 1, h0 - 2, h0 + 3, weak=True)
    assert len(got) == 1 and (got[0]["f0"], got[0]["h0"]) == (f0, h0) and got[0]["word"] in {t["word"] for t in truth}
    assert got[0]["score"] == wc.strongest()[2]
    assert ft4.decode_twin(x, f0, f0 + 1, h0 - 2, h0 + 3, weak=True, weak_min=31.0) == []


# ---- 2. host traces: the setter is called once per _ft4_set, and never without the keyword
class Recorder:
    """A stand-in handle that records the FT4 calls and hands out empty results"""
    calls = []

    def __init__(self, cfg=None, device=0, max_frames=1):
        self.cfg, self.max_frames = cfg, int(max_frames)

    def set_ladder_mode(self, mode):
        pass

    def close(self):
        pass

    def _empty(self, B):
        mc = self.cfg.max_cands
        return (np.zeros((B, mc), _lib.RECORD_DTYPE), np.zeros(B, np.int32), np.zeros((B, _lib.EVENT_CAP), _lib.EVENT_DTYPE), np.zeros(B, np.int32))

    def ft4_set(self, sync_min=None, osd_max_hd=None):
        Recorder.calls.append("ft4_set")

    def ft4_set_range(self, *a):
        Recorder.calls.append("ft4_set_range")

    def ft4_set_coherent(self, on):
        Recorder.calls.append(f"ft4_set_coherent({on})")

    def ft4_set_weak(self, on, weak_min=None):
        Recorder.calls.append(f"ft4_set_weak({on}, {weak_min})")

    def ft4_decode(self, audio):
        Recorder.calls.append(f"ft4_decode({len(audio)})")
        return self._empty(len(audio))

    def ft4_staging_ptr(self):
        return 0x5A5A00

    def ddc_stream_frames(self, m_first, n_have, frame_len, ch):
        Recorder.calls.append(f"ddc_stream_frames({n_have})")

    def ft4_enqueue(self, ptr, B):
        Recorder.calls.append(f"ft4_enqueue({B})")

    def fetch(self, B):
        Recorder.calls.append(f"fetch({B})")
        return self._empty(B)


def take():
    c, Recorder.calls = Recorder.calls, []
    return c


def test_host_traces(monkeypatch):
    monkeypatch.setattr(_lib, "Handle", Recorder)
    take()
    x = np.zeros((2, _lib.FT4_NSAMP), np.int16)
    wide = types.SimpleNamespace(channels={"FT4": [0, 1]}, bands=None, n_channels=2, seen=[{}, {}])
    on = receiver.Receiver("", None, autostart=False, max_frames=2, ft4_weak=True)
    assert on.ft4_weak is True and on.decode_frames_ft4(x) == [[], []]
    assert take() == ["ft4_set", "ft4_set_weak(True, None)", "ft4_set_range", "ft4_decode(2)"]            # before the first pass, once
    for n_have in (72000, _lib.FT4_NSAMP):                                        # the early live pass and the complete one
        out = []
        on._live_pass_ft4(wide, 0, 0, n_have, out)
        assert out == [] and take() == ["ft4_set", "ft4_set_weak(True, None)", "ft4_set_range", f"ddc_stream_frames({n_have})", "ft4_enqueue(2)", "fetch(2)"]
    both = receiver.Receiver("", None, autostart=False, max_frames=2, ft4_weak=True, ft4_coherent=True, ft4_weak_min=16.5)
    assert both.decode_frames_ft4(x) == [[], []]
    assert take() == ["ft4_set", "ft4_set_coherent(True)", "ft4_set_weak(True, 16.5)", "ft4_set_range", "ft4_decode(2)"]
    for kw in ({}, {"ft4_weak": False}):
        off = receiver.Receiver("", None, autostart=False, max_frames=2, **kw)
        assert off.ft4_weak is False and off.decode_frames_ft4(x) == [[], []]
        off._live_pass_ft4(wide, 0, 0, _lib.FT4_NSAMP, [])
        assert take() == ["ft4_set", "ft4_set_range", "ft4_decode(2)", "ft4_set", "ft4_set_range", f"ddc_stream_frames({_lib.FT4_NSAMP})", "ft4_enqueue(2)", "fetch(2)"]
    for bad in (1, 0, "yes", None):
        with pytest.raises(_lib.Ft8rxError, match="ft4_weak must be True or False"):
            receiver.Receiver("", None, autostart=False, ft4_weak=bad)


# ---- 3. the ABI
def test_header_and_prototype_table():
    text = open(os.path.join(ROOT, "include", "ft8rx.h")).read()
    header = c_prototypes(text, r"ft8rx_ft4_(?:set_weak|weak_info|sync_weak)")
    assert sorted(header) == sorted(NEW)
    assert mismatches({n: _abi.PROTOTYPES[n] for n in NEW}, header) == []
    assert [len(_abi.PROTOTYPES[n][1]) for n in NEW] == [3, 4, 9]
    assert all(text.count(n) >= 2 for n in NEW)                                   # the map of the ABI and the declaration
    assert f"#define FT8RX_FT4_WEAK_MIN_DEFAULT   {ft4.WEAK_MIN_DEFAULT:.2f}f" in text


def test_built_library_exports_the_symbols():
    for wide in (False, True):
        for n in NEW:
            assert getattr(_lib.lib(wide), n).argtypes == list(_abi.PROTOTYPES[n][1])
    assert callable(_lib.Handle.ft4_set_weak) and callable(_lib.Handle.ft4_sync_weak) and callable(_lib.Handle.ft4_weak_info)
