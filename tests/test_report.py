"""Measured signal reports (ft8rx_set_reports), the CPU side: the float64 twin pyft8_amd/report.py against
synthetic truth, and the host plumbing.  No GPU.

The accuracy set is the recipe of DESIGN.md section 14: frame i carries ten isolated signals 240 Hz apart, drawn from
np.random.default_rng(100 + i), SNR uniform in -19 .. +15 dB; the oracle decodes it with the default configuration and the twin is
applied to the oracle's cycle spectrum for every decoded true message.  The bounds come from what a report is used for -- an integer
dB, a frequency that rounds to the right Hz, one 5-ms sample -- not from what the estimator gives."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from pyft8_amd import _lib, messages, synth
from pyft8_amd import report as R


def recipe_signals(i):
    """Frame i of the recipe -> [(word, f0 Hz, t0 s, snr dB, text tuple)] for k = 0 .. 9."""
    rng = np.random.default_rng(100 + i)
    out = []
    for k in range(10):
        a, b = synth.random_call(rng), synth.random_call(rng)
        rep = "%+03d" % rng.integers(-20, 10)
        snr = rng.uniform(-19, 15)
        f0 = 400 + 240 * k + rng.uniform(-3, 3)
        t0 = rng.uniform(0, 1.5)
        out.append((synth.pack77(a, b, rep), f0, t0, snr, (a, b, rep)))
    return out


def recipe_frame(i):
    sig = recipe_signals(i)
    return synth.frame_with_signals(7000 + i, [s[:4] for s in sig]), sig


def check_bounds(truth, got, n_signals):
    """truth / got: arrays [n, 3] of (snr dB, f Hz, t s).  Prints every figure, then asserts the bounds of the issue."""
    truth, got = np.asarray(truth, float), np.asarray(got, float)
    e = got - truth
    lo = truth[:, 0] <= 0
    fig = dict(n=len(e), f_mean=e[:, 1].mean(), f_rms=np.sqrt((e[:, 1] ** 2).mean()), t_mean=e[:, 2].mean(), t_std=e[:, 2].std(),
               snr_lo_mean=e[lo, 0].mean(), snr_lo_rms=np.sqrt((e[lo, 0] ** 2).mean()), snr_hi_mean=e[~lo, 0].mean(),
               snr_hi_worst=np.abs(e[~lo, 0]).max(), n_lo=int(lo.sum()), n_hi=int((~lo).sum()))
    print("report accuracy:", {k: (round(float(v), 4) if not isinstance(v, int) else v) for k, v in fig.items()})
    assert len(e) >= n_signals * 100 // 160, fig
    assert abs(fig["f_mean"]) <= 0.1 and fig["f_rms"] <= 0.25, fig
    assert abs(fig["t_mean"]) <= 0.005 and fig["t_std"] <= 0.0025, fig
    assert abs(fig["snr_lo_mean"]) <= 1.0 and fig["snr_lo_rms"] <= 1.5, fig
    assert -3.0 <= fig["snr_hi_mean"] <= 1.0 and fig["snr_hi_worst"] <= 6.0, fig
    return fig


def test_twin_against_truth():
    truth, got = [], []
    for i in range(16):
        audio, sig = recipe_frame(i)
        res = O.decode_frame(audio)
        spec = O.cycle_spectrum(audio)
        by_text = {s[4]: s for s in sig}
        before = [(m["snr"], m["fHz"], m["tsec"]) for m in res["msgs"]]
        for m in res["msgs"]:
            if m["msg_tuple"] not in by_text:
                continue
            w, f0, t0, snr, _ = by_text.pop(m["msg_tuple"])
            c = res["cands"][m["cand"]]
            tt, ft = (m["ttweak"], m["ftweak"]) if m["fine"] else (0, 0)
            assert (c.ttweak, c.ftweak) == (tt, ft) or not m["fine"]
            r = R.measure(spec, c.f0_idx, c.h0_idx, tt, ft, w)
            assert r is not None and r["flags"] & R.MEASURED
            truth.append((snr, f0, t0))
            got.append((r["snr_db"], r["f_hz"], r["t_sec"]))
        # the measurement reads the spectrum and the record, and leaves the reference's quantities as they are
        assert before == [(m["snr"], m["fHz"], m["tsec"]) for m in O.decode_frame(audio)["msgs"]] == [(m["snr"], m["fHz"], m["tsec"]) for m in res["msgs"]]
    check_bounds(truth, got, 160)


def test_twin_definition_pieces():
    """The pieces of the definition on small inputs: the tones, the far-cell mask, the median, the parabola, validity."""
    w = synth.pack77("K1ABC", "W9XYZ", "-05")
    tones = synth.tones79(w)
    far = R.far_mask(tones)
    assert far.shape == (79, 8)
    for s in range(79):
        for t in range(8):
            near = any(abs(t - tones[q]) <= 2 for q in (s - 1, s, s + 1) if 0 <= q < 79)
            assert far[s, t] == (not near)
    assert R.median([3.0, 1.0, 2.0]) == 2.0 and R.median([4.0, 1.0, 2.0, 3.0]) == 2.5
    assert R._parabola(1.0, 2.0, 1.0) == 0.0 and R._parabola(1.0, 2.0, 2.0) == pytest.approx(0.5)
    assert abs(float((R.HANN ** 2).sum()) - 12.0) < 1e-12
    spec = np.zeros(_lib.SPEC_BINS, np.complex64)
    assert R.measure(spec, 100, _lib.MIN_H0_FD - 1, 0, 0, w) is None
    assert R.measure(spec, 100, _lib.MAX_H0_FD + 1, 0, 0, w) is None
    assert R.measure(spec, 2, 10, 0, 0, w) is None                       # fb - 150 < 0
    assert R.measure(spec, 983, 10, 0, 0, w) is None                     # fb + 850 beyond the spectrum
    # a noise-free tone sequence placed on the series: the scan finds its sample and its frequency offset
    z = np.zeros(3200, complex)
    n = np.arange(32)
    for s, t in enumerate(tones):
        z[500 + 32 * s:532 + 32 * s] = np.exp(2j * np.pi * n * (t + 0.23) / 32)
    P = R.scan(z, tones, 510)
    it, idl = np.unravel_index(int(np.argmax(P)), P.shape)
    assert 510 + R.TAU_LO + it == 500 and idl == 9                       # delta = +0.2 is the nearest scan point


def test_abi_and_refusals():
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_WIDE):
        L = C.CDLL(path)
        for s in ("ft8rx_set_reports", "ft8rx_fetch_reports", "ft8rx_report_probe"):
            assert hasattr(L, s), (path, s)
    assert _lib.REPORT_DTYPE.itemsize == 24
    assert (R.MEASURED, R.INVALID, R.EDGE_T, R.EDGE_F) == (_lib.RP_MEASURED, _lib.RP_INVALID, _lib.RP_EDGE_T, _lib.RP_EDGE_F)
    from pyft8_amd.receiver import config_from_kwargs
    cfg = config_from_kwargs()
    assert cfg.reports is False


def test_message_dicts_carry_the_report():
    """message_dicts(..., reports=) looks the report up by the message's cand, gives None for an invalid one and for a recall message,
    and leaves every other key as it is."""
    msgs = np.zeros(4, _lib.MESSAGE_DTYPE)
    for i, (text, cand, ipass) in enumerate(((("K1ABC", "W9XYZ", "-05"), 2, 4), (("CQ", "G4XYZ", "IO91"), 0, 0), (("A1AA", "B2BB", "73"), 1, 5),
                                             (("K1ABC", "W9XYZ", "RR73"), 3, 8))):
        msgs[i]["f"] = [t.encode() for t in text]
        msgs[i]["cand"], msgs[i]["ipass"], msgs[i]["f0_idx"], msgs[i]["h0_idx"], msgs[i]["fine"] = cand, ipass, 300 + i, 10 + i, ipass >= 4
    rp = np.zeros(5, _lib.REPORT_DTYPE)
    rp[0] = (-3.5, 940.2, 0.41, 1.0, _lib.RP_MEASURED, 0)
    rp[1] = (np.nan, np.nan, np.nan, np.nan, _lib.RP_MEASURED | _lib.RP_INVALID, 0)
    rp[2] = (7.25, 938.9, 0.52, 2.0, _lib.RP_MEASURED | _lib.RP_EDGE_F, 0)
    rp[3] = (1.0, 1.0, 1.0, 1.0, _lib.RP_MEASURED, 0)
    plain = messages.message_dicts(msgs, 4, cyclestart_string="x")
    with_r = messages.message_dicts(msgs, 4, cyclestart_string="x", reports=rp)
    assert [d["report"] for d in with_r] == [{"snr": 7.25, "fHz": pytest.approx(938.9), "tsec": pytest.approx(0.52)},
                                             {"snr": -3.5, "fHz": pytest.approx(940.2), "tsec": pytest.approx(0.41)}, None, None]
    for a, b in zip(plain, with_r):
        assert "report" not in a
        assert {k: v for k, v in b.items() if k not in ("report", "decode_completed")} == {k: v for k, v in a.items() if k != "decode_completed"}
