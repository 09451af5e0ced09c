"""Weak mode (ft8rx_set_weak) without a GPU: the receiver kwargs and their refusals, the library's exports and
defaults, and the numpy twin (tests/weak_twin.py) against the oracle where the two overlap."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import weak_twin as W
from conftest import ROOT
from pyft8_amd import _lib, synth
from pyft8_amd.receiver import config_from_kwargs


def test_kwargs():
    c = config_from_kwargs()
    assert not c.weak and c.weak_sync_min is None and c.weak_osd_max_hd is None
    c = config_from_kwargs(weak=True, weak_sync_min=160, weak_osd_max_hd=38)
    assert c.weak and c.weak_sync_min == 160.0 and c.weak_osd_max_hd == 38
    for f in _lib.Config._fields_:                   # the frozen ft8rx_config is untouched: a handle setting, not a field
        assert getattr(c, f[0]) == getattr(config_from_kwargs(), f[0])


@pytest.mark.parametrize("kw, match", [
    (dict(weak=True, msg_types="all"), "msg_types"),
    (dict(weak=True, my_call="K1ABC"), "my_call"),
    (dict(weak=True, dx_call="K1ABC"), "my_call"),
    (dict(weak_sync_min=150), "weak=True"),
    (dict(weak=True, weak_sync_min=0), "weak_sync_min"),
    (dict(weak=True, weak_sync_min=float("nan")), "weak_sync_min"),
    (dict(weak=True, weak_osd_max_hd=175), "weak_osd_max_hd"),
])
def test_kwarg_refusals(kw, match):
    with pytest.raises(_lib.Ft8rxError, match=match):
        config_from_kwargs(**kw)


def test_header_and_exports():
    h = open(os.path.join(ROOT, "include", "ft8rx.h")).read()
    assert float(re.search(r"FT8RX_WEAK_SYNC_MIN_DEFAULT ([0-9.]+)f", h).group(1)) == _lib.WEAK_SYNC_MIN_DEFAULT
    assert int(re.search(r"FT8RX_WEAK_OSD_MAX_HD_DEFAULT (\d+)", h).group(1)) == _lib.WEAK_OSD_MAX_HD_DEFAULT
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_WIDE):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for s in ("ft8rx_set_weak", "ft8rx_sync_scores_weak", "ft8rx_fine_weak"):
            assert re.search(r"\b" + s + r"\b", syms), (path, s)


def test_twin_middle_block_is_the_oracle_search():
    """The twin's row rules (wrap, 1.0 outside the cycle) and fp64 order, restricted to the middle block, give the oracle's search."""
    a = synth.make_frame(5, n_signals=20, snr_range=(-15.0, 5.0))
    ocfg = W.oracle_config()
    g = O.spectrogram(a, ocfg)
    f0, h0 = np.arange(ocfg.f0_lo, ocfg.f0_hi), np.arange(ocfg.h0_lo, ocfg.h0_hi)
    s1 = np.zeros((len(h0), len(f0)))
    ts = np.zeros_like(s1)
    for s in range(7):
        R = W._rows(g, h0 + 148 + 4 * s)
        t = np.zeros_like(s1)
        for k in range(14):
            t = t + R[:, f0 + k]
        ts = ts + t
        c = W.COSTAS[s]
        s1 = s1 + (R[:, f0 + 2 * c] + R[:, f0 + 2 * c + 1])
    sc = (s1 + W.W6 * (ts - s1)).astype(np.float32)
    best, bh = np.zeros(len(f0), np.float32), np.zeros(len(f0), np.int32)
    for i in range(len(h0)):
        m = sc[i] > best
        best, bh = np.where(m, sc[i], best), np.where(m, h0[i], bh)
    keep = sorted([(int(f0[i]), int(bh[i]), float(best[i])) for i in range(len(f0)) if best[i] > np.float32(85)], key=lambda c: -c[2])
    ref = [(c.f0_idx, c.h0_idx, float(np.float32(c.score))) for c in O.sync_search(g, ocfg)]
    assert keep[:ocfg.max_cands] == ref


def test_twin_three_block_score_finds_weak_signals():
    """At -21 dB the three-block search keeps more of the true signals than the reference's one-block search."""
    ocfg = W.oracle_config()
    hit1 = hit3 = 0
    for i in range(3):
        a, tr = synth.make_frame(40 + i, n_signals=10, snr_range=(-21.0, -21.0), return_truth=True)
        g = O.spectrogram(a, ocfg)
        one = {c.f0_idx for c in O.sync_search(g, ocfg)}
        three = {c[0] for c in W.search(g, ocfg, _lib.WEAK_SYNC_MIN_DEFAULT)}
        for t in tr:
            near = set(range(int(t["f0"] / 3.125) - 2, int(t["f0"] / 3.125) + 3))
            hit1 += bool(near & one)
            hit3 += bool(near & three)
    assert hit3 > hit1


def test_twin_fine_weak_at_zero_tweak_is_the_reference_grid():
    """The twin's joint scan returns the reference-defined grid of its chosen tweaks, and scores no lower than the (0, 0) tweak."""
    a, tr = synth.make_frame(9, n_signals=5, snr_range=(-12.0, -12.0), return_truth=True)
    ocfg = W.oracle_config()
    spec = O.cycle_spectrum(a, ocfg)
    c = W.search(O.spectrogram(a, ocfg), ocfg, _lib.WEAK_SYNC_MIN_DEFAULT)[0]
    r = W.fine_weak(spec, c[0], c[1], ocfg)
    fb0, tb0 = 50 * c[0], 8 * c[1] + (c[1] < 0)
    assert r["score"] >= W.score3(W.fine_grid(spec, fb0, tb0, ocfg))
    assert r["sgrid"].tobytes() == W.fine_grid(spec, fb0 + r["ftweak"], tb0 + r["ttweak"], ocfg).tobytes()
    assert r["nsync"] > 6 and r["ret"] == 1
