"""FT4 coherent LLRs on the GPU (k_ft4_coh and the opt-in step of the FT4 chain): the stage against the float64
twin ft4.coherent_llrs, the setting off = the chain as it was, on with strong and with weak signals, with subtraction passes and a small
max_cands.  Run with -m gpu on an MI355X."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import ft4_cases as cases
from pyft8_amd import _lib, ft4, synth
from pyft8_amd.receiver import Receiver, decode_frames_ft4
from test_gpu_ft4 import LLR_BOUND, METRIC_BOUND

pytestmark = pytest.mark.gpu
# A run adds at most four of the demodulator's sums and a maximum is 1-Lipschitz in them: 4 x the demodulator's bounds
COH_METRIC_BOUND = 4 * METRIC_BOUND
COH_LLR_BOUND = 4 * LLR_BOUND
Q_GAP = 1e-5                          # q is compared wherever the twin's best two metrics lie further apart than this, relative


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


# ----------------------------------------------------------------------------- 1. the stage against the twin
def test_stage_against_the_twin():
    audio, cands = cases.demod_candidates(65)
    tw = [cases.twin_demod(*c) for c in cands]
    h = _lib.Handle(max_frames=3)
    try:
        got = h.ft4_coherent(audio, [c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands], [t["tt"] for t in tw], [t["ft"] for t in tw])
        assert h.ft4_coh_info() == dict(workspace_bytes=0, on=False)              # the stage entry owns nothing of the chain's
    finally:
        h.close()
    assert np.isfinite(got["llr2"]).all() and np.isfinite(got["llr4"]).all() and np.isfinite(got["metrics"]).all()
    worst_m, worst_l, compared = 0.0, 0.0, 0
    for i, (c, t) in enumerate(zip(cands, tw)):
        ref = ft4.coherent_llrs(audio[c[0]], c[1], c[2], t["tt"], t["ft"])
        m = np.sort(ref["metrics"])
        if m[-1] == 0.0:                                                        # the all-zero frame: exactly the twin
            assert c[0] == 2 and int(got["q"][i]) == ref["q"] == -4 and not got["metrics"][i].any() and not got["llr2"][i].any() and not got["llr4"][i].any()
            continue
        clear = m[-1] - m[-2] > Q_GAP * m[-1]
        assert clear or c[0] == 1, c                                           # only a noise candidate may be excused: the four signal families never are
        if clear:
            assert int(got["q"][i]) == ref["q"], c
            compared += 1
        worst_m = max(worst_m, np.abs(got["metrics"][i] - ref["metrics"]).max() / m[-1])
        if int(got["q"][i]) == ref["q"]:
            for k in ("llr2", "llr4"):
                worst_l = max(worst_l, np.abs(got[k][i] - ref[k]).max() / np.abs(ref[k]).max())
    print(f"ft4 coherent stage, 65 candidates: metrics {worst_m:.3e}, llr {worst_l:.3e}, q compared on {compared}")
    assert compared >= 60 and worst_m <= COH_METRIC_BOUND and worst_l <= COH_LLR_BOUND


# ----------------------------------------------------------------------------- 2. off is the chain as it was
def test_off_is_the_parent():
    six = np.stack([cases.six(i)[0] for i in cases.SIX])
    crafted = cases.demod_frames()[0]
    ft8 = synth.make_frame(7, n_signals=12, snr_range=(-12.0, 5.0))
    never, toggled, fresh = _lib.Handle(max_frames=3), _lib.Handle(max_frames=3), _lib.Handle(max_frames=3)
    try:
        a = [never.ft4_decode(x) for x in (six, crafted)]
        base = never.ft4_info()["workspace_bytes"]
        assert never.ft4_coh_info() == dict(workspace_bytes=0, on=False)
        toggled.ft4_set_coherent(True)
        assert toggled.ft4_coh_info() == dict(workspace_bytes=0, on=True)        # nothing until a batch runs with it
        toggled.ft4_decode(crafted)
        info = toggled.ft4_coh_info()
        assert info["on"] and info["workspace_bytes"] > 2 * 174 * 4 * (3 << 8) and toggled.ft4_info()["workspace_bytes"] == base
        toggled.ft4_set_coherent(False)
        assert toggled.ft4_coh_info() == dict(workspace_bytes=info["workspace_bytes"], on=False)
        for x, want in zip((six, crafted), a):
            _same(toggled.ft4_decode(x), want)
            _same(fresh.ft4_decode(x), want)
        assert fresh.ft4_coh_info()["workspace_bytes"] == 0 and never.ft4_coh_info()["workspace_bytes"] == 0
        # FT8 behind a coherent FT4 batch
        toggled.ft4_set_coherent(True)
        toggled.ft4_decode(six)
        clean = _lib.Handle(max_frames=3)
        try:
            _same(toggled.decode_batch(ft8), clean.decode_batch(ft8))
        finally:
            clean.close()
    finally:
        never.close(); toggled.close(); fresh.close()


# ----------------------------------------------------------------------------- 3. on, strong signals: everything decodes before the new step
def test_on_strong_signals_changes_nothing():
    six = np.stack([cases.six(i)[0] for i in cases.SIX])
    quiet = np.stack([cases.noise_frame(), cases.zero_frame()])
    off, on = _lib.Handle(max_frames=3), _lib.Handle(max_frames=3)
    try:
        on.ft4_set_coherent(True)
        a, b = off.ft4_decode(six), on.ft4_decode(six)
        _same(a, b)
        st = np.concatenate([a[0][f, :int(a[1][f])]["status"] for f in range(3)])
        assert (st == _lib.ST_DECODED).sum() >= 18 and not b[0]["nsync"].any()
        a, b = off.ft4_decode(quiet), on.ft4_decode(quiet)
        _same(a, b)
        n = int(b[1][0])
        assert n >= 1 and (b[0][0, :n]["status"] == _lib.ST_EXHAUSTED).all() and int(b[1][1]) == 0
    finally:
        off.close(); on.close()


# ----------------------------------------------------------------------------- 4. on, weak signals
@functools.lru_cache(maxsize=None)
def weak_frames():
    fr = [ft4.make_frame(155000 + i, n_signals=10, snr_range=(-15.5, -15.5), min_sep_hz=150, return_truth=True) for i in range(8)]
    return np.stack([f[0] for f in fr]), [{t["msg"] for t in f[1]} for f in fr]


def test_on_weak_signals():
    audio, planted = weak_frames()
    rx_off, rx_on = Receiver("", None, max_frames=8), Receiver("", None, max_frames=8, ft4_coherent=True)
    try:
        off = rx_off.decode_frames_ft4(audio)
        on, rec, cnt = rx_on.decode_frames_ft4(audio, return_records=True)
        n_off, n_on = sum(len(x) for x in off), sum(len(x) for x in on)
        print(f"ft4 coherent, 8 frames of 10 signals at -15.5 dB: {n_off} messages off, {n_on} on")
        hit = None
        for f in range(8):
            assert set(_texts(off[f])) <= set(_texts(on[f])), f                # every off message is among the on messages
            assert set(_texts(on[f])) <= planted[f], f                         # every on message is a planted text
            assert all("nsym" not in d for d in off[f]) and all(d["nsym"] in (1, 2, 4) for d in on[f])
            r = rec[f, :int(cnt[f])]
            coh = r[(r["status"] == _lib.ST_DECODED) & (r["nsync"] != 0)]
            assert np.isin(coh["nsync"], (2, 4)).all() and (coh["ipass"] == 4).all() and (coh["method"] == _lib.M_LDPC_B).all() and not coh["ap"].any()
            # a dict says the run length of the record it was made from: the decoded record at the dict's start and frequency
            dec = r[r["status"] == _lib.ST_DECODED]
            at = {((ft4.HOP * int(x["h0_idx"]) + ft4.DT_STEP * int(x["ttweak"])) / ft4.FS, ft4.BIN_HZ * int(x["f0_idx"]) + ft4.DF_HZ * int(x["ftweak"])):
                  int(x["nsync"]) or 1 for x in dec}
            assert len(at) == len(dec) and all(d["nsym"] == at[(d["tsec"], d["fHz"])] for d in on[f]), f
            if any(d["nsym"] != 1 for d in on[f]) and hit is None:
                hit = f
        assert n_on > n_off and hit is not None                                    # strictly more, and a coherent decode with its dict
        # a frame alone gives the records it has in the batch, byte for byte
        one, rec1, cnt1 = rx_on.decode_frames_ft4(audio[hit], return_records=True)
        assert int(cnt1[0]) == int(cnt[hit]) and rec1[0, :int(cnt1[0])].tobytes() == rec[hit, :int(cnt[hit])].tobytes()
        assert _texts(one[0]) == _texts(on[hit]) and sorted(d["nsym"] for d in one[0]) == sorted(d["nsym"] for d in on[hit])
    finally:
        rx_off.close(); rx_on.close()


@pytest.mark.parametrize("kw", [dict(ft4_passes=2), dict(max_cands=2)])
def test_on_with_passes_and_small_max_cands(kw):
    audio, planted = weak_frames()
    audio, planted = audio[:3], planted[:3]
    single = decode_frames_ft4(audio, **{k: v for k, v in kw.items() if k != "ft4_passes"}, ft4_coherent=True)
    got = decode_frames_ft4(audio, ft4_coherent=True, **kw)
    for f in range(3):
        assert set(_texts(got[f])) <= planted[f] and set(_texts(single[f])) <= set(_texts(got[f])), f
        assert all(d["nsym"] in (1, 2, 4) for d in got[f])
    if "max_cands" in kw:
        assert all(len(g) <= 2 for g in got)
