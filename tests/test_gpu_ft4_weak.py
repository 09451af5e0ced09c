"""The FT4 weak search on the GPU (k_ft4_cgrid, k_ft4_csync and the opt-in step of the FT4 chain): the stage
against the float64 twin ft4.search_weak on the fixtures of tests/ft4_weak_cases.py, the setting off = the chain as it was, on with
strong and with weak signals, and with the other FT4 knobs.  Run with -m gpu on an MI355X.

The stage's bound is not this kernel's own error: it is the parent's asserted bound of the same 576-point fp32 LDS FFT (AMP_BOUND =
6e-7 of a row's norm, tests/test_gpu_ft4.py), carried through the score's definition (ft4_weak_cases.score_bound):
    |score - twin| <= (8 D1 + score D2) / (nrm - D2) + |score| 2^-23,
D1 = the sum over the 16 sync rows of d_r, D2 = sqrt(4 sum d_r^2), d_r = 6e-7 x 24 ||x_r||_2, nrm = sqrt(the 64 |W|^2 summed); the last
term is the rounding of the float32 the kernel stores.  On the fixtures that is at most 1.0e-3 of a score between 0 and 32.
best_h0 and the lists are compared wherever the twin's decision is further from a tie than twice that bound: every list decision is
(tests/test_ft4_weak.py asserts it without a GPU), and so are all but 2, 3 and 1 of the 565 per-bin h0 decisions of the signal, noise and
edge frames -- those six bins are left out and counted."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import ft4_cases as cases
import ft4_weak_cases as wc
from pyft8_amd import _lib, ft4, synth
from pyft8_amd.receiver import Receiver, decode_frames_ft4

pytestmark = pytest.mark.gpu
F0, H0 = cases.F0_RANGE, cases.H0_RANGE


def _texts(msgs):
    return sorted(" ".join(x for x in m["msg_tuple"] if x) for m in msgs)


def _events(ev, evc, f):
    return sorted(e.tobytes() for e in ev[f, :int(evc[f])])                    # the log's order is the atomics' (kernels/common.hpp)


def _same(a, b):
    """two dense results of one batch: counts, live records and events (as sets) byte for byte"""
    assert a[1].tobytes() == b[1].tobytes() and a[3].tobytes() == b[3].tobytes()
    for f in range(len(a[1])):
        n = int(a[1][f])
        assert a[0][f, :n].tobytes() == b[0][f, :n].tobytes(), f
        assert _events(a[2], a[3], f) == _events(b[2], b[3], f), f


def _check_frame(name, t, f0_lo, max_cands, f0, h0, sc, cnt, bs, bh):
    """one frame of a stage result against the twin's dict t -> the number of bins left out of the h0 comparison"""
    want = wc.twin_list(t, f0_lo, wc.STAGE_WEAK_MIN, max_cands)
    n = int(cnt)
    assert [(int(a), int(b)) for a, b in zip(f0[:n], h0[:n])] == [c[:2] for c in want], name
    bb = wc.best_bound(t)
    err = np.abs(bs.astype(np.float64) - t["best"])
    print(f"ft4 weak stage {name}, max_cands {max_cands}: {n} candidates, best off by at most {err.max():.3e} (bound {bb.max():.3e}, "
          f"worst share of its bound {np.max(err / np.maximum(bb, 1e-300)) if bb.max() > 0 else 0.0:.3f})")
    assert np.all(err <= bb), name
    for k, c in enumerate(want):
        assert abs(float(sc[k]) - c[2]) <= bb[c[0] - f0_lo], (name, c)
    if not t["best"].any():                                                    # digital silence: exact zeros, the first h0 of the range
        assert not bs.any() and np.array_equal(bh, t["bh"]) and n == 0
        return 0
    clear = wc.h0_clear(t)
    assert np.array_equal(bh[clear], t["bh"][clear]), name
    return int((~clear).sum())


# ----------------------------------------------------------------------------- 1. the stage against the twin
@pytest.mark.parametrize("max_cands", [4, 256])
def test_stage_against_the_twin(max_cands):
    h = _lib.Handle(_lib.default_config(max_cands=max_cands), max_frames=3)
    try:
        h.ft4_set_weak(True, wc.STAGE_WEAK_MIN)
        names = wc.FRAMES[:3]
        got = h.ft4_sync_weak(np.stack([wc.frame(n) for n in names]), want_best=True)
        left = sum(_check_frame(n, wc.twin(n), F0[0], max_cands, *(g[f] for g in got)) for f, n in enumerate(names))
        h.ft4_set_range(F0[0], F0[1], *wc.H0_WIDE)                              # the edge frame: a signal from -0.3 s, one past the frame's end
        got = h.ft4_sync_weak(wc.frame("edges"), want_best=True)
        left += _check_frame("edges", wc.twin("edges"), F0[0], max_cands, *(g[0] for g in got))
        print(f"ft4 weak stage: {left} of {4 * (F0[1] - F0[0])} h0 decisions left out (closer to a tie than twice the bound)")
        assert left <= 6
        if max_cands == 256:                                                    # the lowest and the highest f0 of the range are candidates
            n = int(got[3][0])
            assert {F0[0], F0[1] - 1} <= set(int(v) for v in got[0][0, :n])
        # a frame alone: the same bits as in the batch
        h.ft4_set_range()
        one = h.ft4_sync_weak(wc.frame("noise"), want_best=True)
        three = h.ft4_sync_weak(np.stack([wc.frame(n) for n in names]), want_best=True)
        assert all(np.array_equal(a[0], b[1]) for a, b in zip(one, three))
    finally:
        h.close()


def test_stage_in_narrow_ranges():
    """one f0 bin, and the whole band with the h0 range narrowed to one row: the strongest planted signal alone"""
    h = _lib.Handle(max_frames=3)
    try:
        h.ft4_set_weak(True, wc.STAGE_WEAK_MIN)
        for rng in wc.narrow_ranges():
            h.ft4_set_range(*rng)
            got = h.ft4_sync_weak(wc.frame("six signals"), want_best=True)
            assert got[4].shape == (1, rng[1] - rng[0])
            assert _check_frame(f"six signals in {rng}", wc.twin("six signals", *rng), rng[0], 256, *(g[0] for g in got)) == 0
            assert int(got[3][0]) == 1 and (int(got[0][0, 0]), int(got[1][0, 0])) == wc.strongest()[:2]
        f0, h0, _ = wc.strongest()
        h.ft4_set_range(f0 + 2, f0 + 3, h0, h0 + 1)                             # one tone off, one row: far below the threshold
        assert int(h.ft4_sync_weak(wc.frame("six signals"))[3][0]) == 0
    finally:
        h.close()


# ----------------------------------------------------------------------------- 2. off is the chain as it was
def test_off_is_the_parent():
    six = np.stack([cases.six(i)[0] for i in cases.SIX])
    crafted = cases.demod_frames()[0]
    ft8 = synth.make_frame(7, n_signals=12, snr_range=(-12.0, 5.0))
    never, toggled, fresh = _lib.Handle(max_frames=3), _lib.Handle(max_frames=3), _lib.Handle(max_frames=3)
    try:
        a = [never.ft4_decode(x) for x in (six, crafted)]
        base, coh = never.ft4_info()["workspace_bytes"], never.ft4_coh_info()
        wm = float(np.float32(ft4.WEAK_MIN_DEFAULT))
        assert never.ft4_weak_info() == dict(workspace_bytes=0, on=False, weak_min=wm)
        toggled.ft4_set_weak(True)
        assert toggled.ft4_weak_info() == dict(workspace_bytes=0, on=True, weak_min=wm)          # nothing until a batch runs with it
        toggled.ft4_decode(crafted)
        info = toggled.ft4_weak_info()
        assert info["on"] and info["workspace_bytes"] == 8 * (3 * 628 * 2306 + 5 * 576 + 32)
        assert toggled.ft4_info()["workspace_bytes"] == base and toggled.ft4_coh_info() == coh
        toggled.ft4_set_weak(False)
        assert toggled.ft4_weak_info() == dict(workspace_bytes=info["workspace_bytes"], on=False, weak_min=wm)
        for x, want in zip((six, crafted), a):
            _same(toggled.ft4_decode(x), want)
            _same(fresh.ft4_decode(x), want)
        assert fresh.ft4_weak_info()["workspace_bytes"] == 0 and never.ft4_weak_info()["workspace_bytes"] == 0
        # FT8 behind a weak FT4 batch
        toggled.ft4_set_weak(True)
        toggled.ft4_decode(six)
        clean = _lib.Handle(max_frames=3)
        try:
            _same(toggled.decode_batch(ft8), clean.decode_batch(ft8))
        finally:
            clean.close()
    finally:
        never.close(); toggled.close(); fresh.close()


# ----------------------------------------------------------------------------- 3. on, strong signals
def test_on_strong_signals():
    frames = [cases.six(i) for i in cases.SIX]
    audio = np.stack([f[0] for f in frames])
    rx = Receiver("", None, max_frames=3, ft4_weak=True)
    try:
        out, rec, cnt = rx.decode_frames_ft4(audio, return_records=True)
        for f, (x, truth) in enumerate(frames):
            assert _texts(out[f]) == sorted(t["msg"] for t in truth)            # the planted texts and nothing else
            by = {" ".join(m["msg_tuple"]): m for m in out[f]}
            for t in truth:
                m = by[t["msg"]]
                assert abs(m["tsec"] - t["t0"]) <= 0.005 and abs(m["fHz"] - t["f0"]) <= 3.0, (t, m["tsec"], m["fHz"])
                assert m["mode"] == "FT4" and "nsym" not in m and "report" not in m
            one, rec1, cnt1 = rx.decode_frames_ft4(x, return_records=True)      # a frame alone: its records in the batch, byte for byte
            assert _texts(one[0]) == _texts(out[f]) and int(cnt1[0]) == int(cnt[f])
            assert rec1[0, :int(cnt1[0])].tobytes() == rec[f, :int(cnt[f])].tobytes()
            r = rec[f, :int(cnt[f])]
            assert (r["score"] >= ft4.WEAK_MIN_DEFAULT).all() and (r["score"] <= 32.0).all() and np.array_equal(r["grid_sd"], r["score"])
        assert rx.decode_frames_ft4(np.stack([cases.zero_frame(), cases.noise_frame()])) == [[], []]
    finally:
        rx.close()


# ----------------------------------------------------------------------------- 4. on, weak signals
@functools.lru_cache(maxsize=None)
def weak_frames():
    fr = [ft4.make_frame(165000 + i, n_signals=10, snr_range=(-16.5, -16.5), min_sep_hz=150, return_truth=True) for i in range(8)]
    return np.stack([f[0] for f in fr]), [{t["msg"] for t in f[1]} for f in fr]


def test_on_weak_signals():
    audio, planted = weak_frames()
    rx_off, rx_on = Receiver("", None, max_frames=8, ft4_coherent=True), Receiver("", None, max_frames=8, ft4_coherent=True, ft4_weak=True)
    try:
        off, on = rx_off.decode_frames_ft4(audio), rx_on.decode_frames_ft4(audio)
        n_off, n_on = sum(len(x) for x in off), sum(len(x) for x in on)
        print(f"ft4 weak search, 8 frames of 10 signals at -16.5 dB, coherent LLRs on: {n_off} messages off, {n_on} on")
        for f in range(8):
            assert set(_texts(off[f])) <= planted[f] and set(_texts(on[f])) <= planted[f], f         # no wrong text in either
        assert n_on >= n_off                                                       # not fewer
    finally:
        rx_off.close(); rx_on.close()


# ----------------------------------------------------------------------------- 5. with the other knobs
@pytest.mark.parametrize("kw", [dict(ft4_passes=2), dict(max_cands=2)])
def test_on_with_passes_and_small_max_cands(kw):
    audio, planted = weak_frames()
    audio, planted = audio[:3], planted[:3]
    single = decode_frames_ft4(audio, **{k: v for k, v in kw.items() if k != "ft4_passes"}, ft4_weak=True)
    got = decode_frames_ft4(audio, ft4_weak=True, **kw)
    for f in range(3):
        assert set(_texts(got[f])) <= planted[f] and set(_texts(single[f])) <= set(_texts(got[f])), f
    if "max_cands" in kw:
        assert all(len(g) <= 2 for g in got)


def test_on_with_reports():
    """the report of a decode depends on its start, carrier and word alone: where both searches lead to the same three, the rows are equal"""
    frames = [cases.six(i) for i in cases.SIX]
    audio = np.stack([f[0] for f in frames])
    rx_off, rx_on = Receiver("", None, max_frames=3, ft4_reports=True), Receiver("", None, max_frames=3, ft4_reports=True, ft4_weak=True)
    try:
        off, on = rx_off.decode_frames_ft4(audio), rx_on.decode_frames_ft4(audio)
        n = 0
        for f in range(3):
            assert _texts(on[f]) == _texts(off[f]) == sorted(t["msg"] for t in frames[f][1])
            a = {m["msg_tuple"]: m for m in off[f]}
            for m in on[f]:
                p = a[m["msg_tuple"]]
                assert m["report"] is not None and abs(m["report"]["fHz"] - m["fHz"]) <= 2.0
                if (p["tsec"], p["fHz"]) == (m["tsec"], m["fHz"]):
                    assert m["report"] == p["report"]
                    n += 1
        assert n >= 15                                                             # of 18
    finally:
        rx_off.close(); rx_on.close()
