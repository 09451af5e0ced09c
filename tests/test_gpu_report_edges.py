"""k_report (kernels/report.hpp) held to its float64 twin at the edges of its domain, through ft8rx_report_probe:
the crafted cases of tests/report_cases.py (tests/test_report_cases.py shows on the CPU that none of them is a near tie, so nothing
is left out here) -- flags, NaNs, the three fields and the score -- then byte-for-byte invariances, the 512-slot layouts, the wide
build, and the batch path on the two configurations where it had only ever been compared with the probe."""
import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import report_cases as RC
from pyft8_amd import _lib, synth
from pyft8_amd import report as R
from pyft8_amd.receiver import config_from_kwargs

pytestmark = pytest.mark.gpu
BOUNDS = (0.01, 0.05e-3, 0.05)            # Hz, s, dB: test_gpu_report.py: test_matches_twin
# score against the twin's P[it, idl], relative.  Measured on an MI355X over the set: 6.7e-7 at worst (series/-2.00s; 6.6e-7 on the wide
# build); the bound is four times that, rounded up to one digit (the issue's rule, which also caps it at 1e-4)
SCORE_BOUND = 3e-6
f32 = np.float32


def _probe(h, spec, cs, frame_of=None):
    return h.report_probe(spec, *RC.columns(cs, frame_of))


@pytest.fixture(scope="module")
def base():
    """All cases of the default layout in one call on a default handle -> (handle, reports); the reports are left unchanged."""
    sp = RC.spectra()
    h = _lib.Handle(max_frames=len(sp))
    assert not h.wide and h.cfg.max_cands <= 256               # the 256-slot layouts
    try:
        rp = _probe(h, sp, RC.cases())
        rp.setflags(write=False)
        yield h, rp
    finally:
        h.close()


def _against_twin(label, cs, tw, got):
    """Flags, NaNs and the three fields of every case against the twin; the spectrum-end cases against their interior case, byte for
    byte; prints the worst deviation per family."""
    worst = {}
    by = {c[0]: g for c, g in zip(cs, got)}
    for c, g in zip(cs, got):
        name, t = c[0], tw[c[0]]
        assert g["pad"] == 0, name
        if t is None:
            assert int(g["flags"]) == _lib.RP_MEASURED | _lib.RP_INVALID == c[7], name
            assert np.isnan([g["snr_db"], g["f_hz"], g["t_sec"], g["score"]]).all(), (name, g)
            continue
        assert int(g["flags"]) == t["flags"] == c[7], (name, int(g["flags"]), t["flags"])
        err = np.abs([g["f_hz"] - t["f_hz"], g["t_sec"] - t["t_sec"], g["snr_db"] - t["snr_db"]])
        worst[RC.family(name)] = np.maximum(worst.get(RC.family(name), 0.0), err)
        assert (err <= BOUNDS).all(), (name, err, g, {k: v for k, v in t.items() if k != "P"})
    for fam, e in worst.items():
        print(f"report edges ({label}) {fam:12s} worst |f| {e[0]:.2e} Hz, |t| {e[1]:.2e} s, |snr| {e[2]:.2e} dB")
    for name, ref in RC.SAME_AS.items():
        a, b = by[name], by[ref]
        for k in ("snr_db", "t_sec", "score", "flags"):
            assert a[k].tobytes() == b[k].tobytes(), (name, k, a, b)
        assert a["f_hz"] != b["f_hz"]


def test_all_cases_match_the_twin(base):
    _, got = base
    cs, tw = RC.cases(), RC.twin()
    _against_twin("default", cs, tw, got)
    by = {c[0]: (c, g) for c, g in zip(cs, got)}
    # SNR floor: off = 0 from the zero fill
    for name in RC.ON_FLOOR:
        assert abs(float(by[name][1]["snr_db"]) - RC.FLOOR_DB) <= 1e-4, name
    # the all-zero spectrum: the closed forms, evaluated as the kernel does in float32 (each within one unit in the last place)
    for name in ("zero/h0+200", "zero/h0-50"):
        (_, _, f0, h0, tt, ft, _, _), g = by[name]
        fb, tau = 50 * f0 + ft, 8 * h0 + (1 if h0 < 0 else 0) + tt - 28
        assert g["score"] == 0.0 and int(g["flags"]) == 13, (name, g)
        want_f, want_t = f32(0.0625) * f32(fb) + f32(6.25) * (f32(0.1) * f32(-7.0)), f32(0.005) * f32(tau)
        assert abs(g["f_hz"] - want_f) <= np.spacing(want_f) and abs(g["t_sec"] - want_t) <= np.spacing(abs(want_t)), (name, g, want_f, want_t)
        assert abs(float(g["f_hz"]) - (0.0625 * fb - 4.375)) <= BOUNDS[0] and abs(float(g["t_sec"]) - 0.005 * tau) <= BOUNDS[1], (name, g)


def _score_deviation(cs, tw, got):
    dev = {c[0]: abs(float(g["score"]) - tw[c[0]]["score"]) / tw[c[0]]["score"] for c, g in zip(cs, got) if tw[c[0]] is not None and tw[c[0]]["score"] > 0.0}
    name = max(dev, key=dev.get)
    return dev, name


def test_score_against_the_twin(base):
    """The score field equals the twin's P[it, idl] within SCORE_BOUND relative on every valid case (0.0 exactly on the all-zero ones)."""
    _, got = base
    cs, tw = RC.cases(), RC.twin()
    dev, name = _score_deviation(cs, tw, got)
    print(f"report edges score: worst relative deviation {dev[name]:.2e} ({name}) over {len(dev)} cases")
    assert len(dev) >= 25
    for n, d in dev.items():
        assert d <= SCORE_BOUND, (n, d)


def test_invariances(base):
    """Byte for byte: the same call twice, the cases in reverse order, each frame's cases alone, and ladder-grid caps 1 and 3 (one
    block walks INVALID and valid items in turn through the same LDS)."""
    h, got = base
    sp, cs = RC.spectra(), RC.cases()
    want = got.tobytes()
    assert _probe(h, sp, cs).tobytes() == want
    assert _probe(h, sp, cs[::-1])[::-1].tobytes() == want
    for s in range(len(sp)):
        idx = [i for i, c in enumerate(cs) if c[1] == s]
        assert idx, s
        alone = _probe(h, sp[s:s + 1], [cs[i] for i in idx], {s: 0})
        assert alone.tobytes() == got[idx].tobytes(), s
    try:
        for cap in (1, 3):
            h.set_ladder_grid(cap)
            assert _probe(h, sp, cs).tobytes() == want, cap
    finally:
        h.set_ladder_grid(0)
    assert _probe(h, sp, cs).tobytes() == want


def test_deep_layouts(base):
    """max_cands = 400: the 512-slot stride, frame = c >> 9.  The interior and border cases in frames 1 and 2 of three give the default
    handle's bytes."""
    _, got = base
    sp, cs = RC.spectra(), RC.cases()
    idx = [i for i, c in enumerate(cs) if c[1] in (0, 1) and RC.family(c[0]) in ("interior", "tborder", "fborder", "bothborders")]
    assert len(idx) == 18
    spec3 = np.stack([np.zeros_like(sp[0]), sp[0], sp[1]])
    h = _lib.Handle(config_from_kwargs(max_cands=400), max_frames=3)
    try:
        assert not h.wide and h.cfg.max_cands == 400
        deep = _probe(h, spec3, [cs[i] for i in idx], {0: 1, 1: 2})
    finally:
        h.close()
    assert deep.tobytes() == got[idx].tobytes()


def test_wide_build():
    """libft8rx_wide.so against the twin on 96000-bin spectra: interior, borders, the spectrum's ends (the last valid slice starts at
    fb = 95150) and a signal at 4500 Hz."""
    sp, cs, tw = RC.spectra(True), RC.cases(True), RC.twin(True)
    h = _lib.Handle(_lib.default_config(f0_hi=1800), max_frames=len(sp))
    try:
        assert h.wide and h.spec_bins == 96000
        got = _probe(h, sp, cs)
        again = _probe(h, sp, cs[::-1])[::-1]
    finally:
        h.close()
    assert got.tobytes() == again.tobytes()
    _against_twin("wide", cs, tw, got)
    by = {c[0]: c for c in cs}
    assert 50 * by["specend/lo-last"][2] + by["specend/lo-last"][5] == 95150 and tw["interior/above3k"]["f_hz"] > 3000.0
    dev, name = _score_deviation(cs, tw, got)
    print(f"report edges score (wide): worst relative deviation {dev[name]:.2e} ({name})")
    assert max(dev.values()) <= SCORE_BOUND


def _batch_against_twin(label, cfg, audio):
    """test_matches_twin's rule and bounds for every DECODED record of one batch -> (decodes, left out as ties, their twin f_hz)."""
    h = _lib.Handle(cfg, max_frames=len(audio))
    try:
        h.set_reports(True)
        rec, cnt, _, _ = h.decode_batch(audio)
        rp = h.fetch_reports(len(audio))
        spec = h.cycle_spectrum(audio)
    finally:
        h.close()
    total = left_out = 0
    worst, f_hz = np.zeros(3), []
    for f in range(len(audio)):
        for i in range(int(cnt[f])):
            x, got = rec[f, i], rp[f, i]
            if x["status"] != _lib.ST_DECODED:
                assert not rp[f, i:i + 1].view(np.uint8).any(), (f, i)
                continue
            tw = R.measure(spec[f], int(x["f0_idx"]), int(x["h0_idx"]), int(x["ttweak"]), int(x["ftweak"]), (int(x["msg_hi"]) << 64) | int(x["msg_lo"]))
            total += 1
            if tw is None:
                assert got["flags"] == _lib.RP_MEASURED | _lib.RP_INVALID and np.isnan([got["snr_db"], got["f_hz"], got["t_sec"]]).all()
                continue
            top = np.sort(tw["P"].ravel())[-2:]
            if top[1] - top[0] <= 1e-5 * top[1]:
                left_out += 1
                continue
            assert int(got["flags"]) == tw["flags"], (label, f, i)
            err = np.abs([got["f_hz"] - tw["f_hz"], got["t_sec"] - tw["t_sec"], got["snr_db"] - tw["snr_db"]])
            worst = np.maximum(worst, err)
            assert (err <= BOUNDS).all(), (label, f, i, err, dict(x=x, got=got, tw={k: v for k, v in tw.items() if k != "P"}))
            f_hz.append(tw["f_hz"])
    print(f"report edges batch ({label}): {total} decodes, {left_out} left out as ties; worst |f| {worst[0]:.2e} Hz, |t| {worst[1]:.2e} s, "
          f"|snr| {worst[2]:.2e} dB")
    assert total >= 30 and left_out <= total // 100
    return np.array(f_hz)


def test_batch_path_wide_build():
    """Two frames with signals up to 5.6 kHz decoded on the wide build with reports on: every DECODED record's report against the twin
    on the handle's own 96000-bin spectrum.  (The generator's signals start near the middle between two 5-ms samples, so about one decode
    in a hundred is a tie of two tau cells; on these two frames the CPU oracle's spectrum shows none under 3e-5, and test_matches_twin's
    allowance of 1 % stays as it is.)"""
    audio = synth.make_batch(64720, 2, n_signals=30, freq_range=(200.0, 5600.0))
    f_hz = _batch_against_twin("wide", config_from_kwargs(search_freq_range=[100, 5900]), audio)
    assert (f_hz > 3000.0).sum() >= 5


def test_batch_path_deep_layouts():
    """Two frames decoded at max_cands = 400 (the 512-slot stride) with reports on, against the twin."""
    audio = synth.make_batch(64800, 2, n_signals=30)
    _batch_against_twin("max_cands=400", config_from_kwargs(max_cands=400), audio)
