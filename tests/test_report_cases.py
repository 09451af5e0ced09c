"""The crafted report cases of tests/report_cases.py on the CPU: the float64 twin (pyft8_amd/report.py) gives each case its designed
flags, no case is a near tie, and none moves under a dither of float32 size.  That is the condition under which
tests/test_gpu_report_edges.py may hold k_report to the twin on every case without an allowance for ties.  No GPU."""
import numpy as np
import pytest

import report_cases as RC
from pyft8_amd import _lib, synth
from pyft8_amd import report as R

LAYOUTS = [False, True]
IDS = ["default", "wide"]
# a tenth of the GPU test's bounds (0.01 Hz, 0.05 ms, 0.05 dB)
DITHER_BOUNDS = (1e-3, 5e-6, 5e-3)
DITHER_SIGMA = 3e-7               # of the slice's RMS: float32 round-off of the 3200-point transform


def _valid(wide):
    tw = RC.twin(wide)
    return [(c, tw[c[0]]) for c in RC.cases(wide) if tw[c[0]] is not None]


def _peak(r):
    return np.unravel_index(int(np.argmax(r["P"])), r["P"].shape)


def _first_off(spec, case, r):
    """`off` from all far cells at the twin's peak: the value the SWITCH decision is made on (R.snr returns the one it ends with)."""
    _, _, f0, h0, tt, ft, w, _ = case
    fb = 50 * f0 + ft
    tones = synth.tones79(w)
    z = R.series(np.asarray(spec), fb)
    it, _ = _peak(r)
    tau = 8 * h0 + (1 if h0 < 0 else 0) + tt + R.TAU_LO + it
    delta = (r["f_hz"] - 0.0625 * fb) / 6.25
    E = np.exp(-2j * np.pi * np.arange(32)[None, :] * (np.arange(8)[:, None] + delta) / 32.0)
    hann = np.abs((R._symbols(z, tau) * R.HANN[None, :]) @ E.T) ** 2
    return R.median(hann[R.far_mask(tones)]) * 32.0 / 12.0 / np.log(2.0)


@pytest.mark.parametrize("wide", LAYOUTS, ids=IDS)
def test_twin_gives_the_designed_results(wide):
    tw = RC.twin(wide)
    cs = RC.cases(wide)
    assert len(RC.spectra(wide)) <= 12
    for name, s, f0, h0, tt, ft, w, flags in cs:
        r = tw[name]
        if flags & R.INVALID:
            assert r is None and flags == R.MEASURED | R.INVALID, name
            continue
        assert r is not None and r["flags"] == flags, (name, r and r["flags"])
        it, idl = _peak(r)
        assert bool(flags & R.EDGE_T) == (it in (0, R.NTAU - 1)) and bool(flags & R.EDGE_F) == (idl in (0, R.NDEL - 1)), name
        tb = 8 * h0 + (1 if h0 < 0 else 0) + tt
        if flags & R.EDGE_T:                                     # on the border the time is the border's, exactly
            assert r["t_sec"] == 0.005 * (tb + R.TAU_LO + it), name
        if flags & R.EDGE_F:
            assert r["f_hz"] == 0.0625 * (50 * f0 + ft) + 6.25 * R.DEL_STEP * (idl - R.NDEL // 2), name
    # every family is there; INVALID cases stand between valid ones of the same spectrum
    fam = {RC.family(c[0]) for c in cs}
    assert fam >= {"interior", "tborder", "fborder", "bothborders", "specend", "invalid"}
    for s in {c[1] for c in cs if c[7] & R.INVALID}:
        inv = [bool(c[7] & R.INVALID) for c in cs if c[1] == s]
        assert not inv[0] and not inv[-1] and 0 < sum(inv) < len(inv) - 1, s
    # both sides of the switch, decided on the first `off`
    sp = RC.spectra(wide)
    by = {c[0]: c for c in cs}
    lo, hi = tw["interior/lo"], tw["interior/hi"]
    assert lo["on"] < 0.5 * R.SWITCH * _first_off(sp[0], by["interior/lo"], lo) and hi["on"] > 2.0 * R.SWITCH * _first_off(sp[1], by["interior/hi"], hi)
    # the first and the last valid slice hold the interior case's bins: the same report, f_hz apart by the shift alone
    for name, ref in RC.SAME_AS.items():
        a, b = tw[name], tw[ref]
        assert (a["snr_db"], a["t_sec"], a["score"], a["flags"]) == (b["snr_db"], b["t_sec"], b["score"], b["flags"]), name
        shift = 0.0625 * ((50 * by[name][2] + by[name][5]) - (50 * by[ref][2] + by[ref][5]))
        assert abs((a["f_hz"] - b["f_hz"]) - shift) < 1e-9 and shift != 0.0, name
    assert {by[n][2:6] for n in RC.SAME_AS} >= {(3, RC.H0, RC.TT, 0)}
    last = (_lib.SPEC_BINS_WIDE if wide else _lib.SPEC_BINS) - 850
    assert any(50 * by[n][2] + by[n][5] == last for n in RC.SAME_AS) and any(50 * by[n][2] + by[n][5] == 150 for n in RC.SAME_AS)


def test_default_layout_families():
    """What only the default layout's set holds: INVALID by time, the two ends of the series, the all-zero spectrum, the words."""
    tw, cs = RC.twin(), RC.cases()
    by = {c[0]: c for c in cs}
    assert {RC.family(c[0]) for c in cs} >= {"series", "zero"}
    assert by["invalid/h0-below"][3] == _lib.MIN_H0_FD - 1 and by["invalid/h0-above"][3] == _lib.MAX_H0_FD + 1
    assert {by[n][3] for n in by if RC.family(n) == "series"} >= {_lib.MIN_H0_FD, _lib.MAX_H0_FD}
    # the series cases: samples before 0 resp. beyond 3199 are read; the first four keep a noise estimate, with exact zeros among its cells
    for name in by:
        if RC.family(name) != "series":
            continue
        _, s, f0, h0, tt, ft, w, _ = by[name]
        tau = 8 * h0 + (1 if h0 < 0 else 0) + tt + R.TAU_LO + _peak(tw[name])[0]
        assert tau < -32 or tau + 32 * 79 > 3200 + 32, name
        assert (tw[name]["off"] == 0.0) == (name in RC.ON_FLOOR), name
    assert sum(8 * by[n][3] < -32 * 30 for n in by if RC.family(n) == "series") >= 2          # 35 symbols before sample 0
    for name in RC.ON_FLOOR:
        assert tw[name]["off"] == 0.0 and tw[name]["snr_db"] == RC.FLOOR_DB, name
    for name in ("zero/h0+200", "zero/h0-50"):
        _, s, f0, h0, tt, ft, w, _ = by[name]
        r = tw[name]
        tb = 8 * h0 + (1 if h0 < 0 else 0) + tt
        assert not r["P"].any() and r["score"] == 0.0 and _peak(r) == (0, 0)
        assert r["f_hz"] == pytest.approx(0.0625 * (50 * f0 + ft) - 4.375, abs=1e-9) and r["t_sec"] == 0.005 * (tb - 28)
    assert by["zero/h0+200"][3] > 0 > by["zero/h0-50"][3]
    words = {c[6] for c in cs if not c[7] & R.INVALID}
    assert len(words) >= 4 and any(w >> 64 for w in words) and synth.pack77_ext("TNX BOB 73 GL") in words
    assert len({tuple(synth.tones79(w)) for w in words}) == len(words)


@pytest.mark.parametrize("wide", LAYOUTS, ids=IDS)
def test_no_case_is_a_near_tie(wide):
    """The two largest cells of P differ by more than 1e-5 relative (the all-zero cases are exempt by construction: every cell ties,
    and the first one wins in any arithmetic), and on / (SWITCH off) is further than 1e-3 from 1 at the decision."""
    sp = RC.spectra(wide)
    worst_gap, worst_sw = np.inf, np.inf
    for c, r in _valid(wide):
        if RC.family(c[0]) != "zero":
            top = np.sort(r["P"].ravel())[-2:]
            gap = (top[1] - top[0]) / top[1]
            worst_gap = min(worst_gap, gap)
            assert gap > 1e-5, (c[0], gap)
        for off in {_first_off(sp[c[1]], c, r), r["off"]}:
            if off > 0.0:
                d = abs(r["on"] / (R.SWITCH * off) - 1.0)
                worst_sw = min(worst_sw, d)
                assert d > 1e-3, (c[0], d)
    print(f"near ties ({IDS[wide]}): smallest relative gap of the two best cells {worst_gap:.2e}, smallest |on / (SWITCH off) - 1| {worst_sw:.2e}")


@pytest.mark.parametrize("wide", LAYOUTS, ids=IDS)
def test_stable_under_dither(wide):
    """Five runs of the twin with complex Gaussian noise of 3e-7 of the slice's RMS on the 1000 bins of the slice: the flags stay, and
    f_hz, t_sec and snr_db move by less than a tenth of the GPU test's bounds."""
    sp = RC.spectra(wide)
    rng = np.random.default_rng(14)
    worst = np.zeros(3)
    for c, r in _valid(wide):
        name, s, f0, h0, tt, ft, w, flags = c
        fb = 50 * f0 + ft
        sl = sp[s][fb - 150:fb + 850].astype(np.complex128)
        sigma = DITHER_SIGMA * np.sqrt((np.abs(sl) ** 2).mean())
        for _ in range(5):
            x = sp[s].astype(np.complex128)
            x[fb - 150:fb + 850] = sl + sigma * (rng.standard_normal(1000) + 1j * rng.standard_normal(1000))
            d = R.measure(x, f0, h0, tt, ft, w)
            assert d["flags"] == flags, name
            err = np.abs([d["f_hz"] - r["f_hz"], d["t_sec"] - r["t_sec"], d["snr_db"] - r["snr_db"]])
            worst = np.maximum(worst, err)
            assert (err < DITHER_BOUNDS).all(), (name, err)
    print(f"dither ({IDS[wide]}): worst |f| {worst[0]:.2e} Hz, |t| {worst[1]:.2e} s, |snr| {worst[2]:.2e} dB")


def test_named_cases_catch_three_mutations(monkeypatch):
    """Three one-line mistakes k_report could make, each played through the twin: the named cases move by far more than the GPU test
    allows (or change their flags), so a kernel with the mistake cannot pass there.
      `it > 0` -> `it >= 0` in the peak step:          tborder/lo+40 peaks in cell it = 0 and must carry EDGE_T
      `i < 3200` -> `i <= 3200` in rp_sample:          zero/h0+200 reads sample 3200 in the scan: whatever non-zero value lies there, the
                                                       score is no longer 0.0, the peak no longer cell 0 and the flags no longer 13
      `j < i` -> `j <= i` in rp_median (every rank one too high, the cells below the middle ones are taken):  interior/lo, interior/hi"""
    tw, sp = RC.twin(), RC.spectra()
    by = {c[0]: c for c in RC.cases()}

    def again(name):
        _, s, f0, h0, tt, ft, w, _ = by[name]
        return R.measure(sp[s], f0, h0, tt, ft, w)

    assert _peak(tw["tborder/lo+40"])[0] == 0 and tw["tborder/lo+40"]["flags"] & R.EDGE_T
    assert _peak(tw["tborder/lo-24"])[0] == R.NTAU - 1 and _peak(tw["fborder/lo+90"])[1] == 0 and _peak(tw["fborder/lo-90"])[1] == R.NDEL - 1

    def symbols_one_more(z, tau):                                # sample 3200 taken for part of the series: whatever lies behind it
        idx = tau + 32 * np.arange(79)[:, None] + np.arange(32)[None, :]
        return np.where((idx >= 0) & (idx <= 3200), np.append(z, 1e-3)[np.clip(idx, 0, 3200)], 0.0)
    with monkeypatch.context() as m:
        m.setattr(R, "_symbols", symbols_one_more)
        r = again("zero/h0+200")
        assert r["score"] > 0.0 and _peak(r) != (0, 0) and r["flags"] != tw["zero/h0+200"]["flags"]

    def median_one_low(cells):
        c = np.sort(np.asarray(cells, float))
        return 0.5 * (c[(len(c) - 1) // 2 - 1] + c[len(c) // 2 - 1])
    with monkeypatch.context() as m:
        m.setattr(R, "median", median_one_low)
        for name in ("interior/lo", "interior/hi"):
            assert abs(again(name)["snr_db"] - tw[name]["snr_db"]) > 2 * 0.05, name
