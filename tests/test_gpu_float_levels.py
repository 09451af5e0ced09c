"""The float32 path against the CPU oracle on real floats: frames with full 24-bit mantissas at three levels
(tests/float_frames_cases.py: NORM, QUIET, LOUD; no scale is a power of two), with large samples next to every zero mask.

Stages: spectrogram_f32 and cycle_spectrum_f32 bit for bit against O.spectrogram_f32 and O.cycle_spectrum_f32, default and wide build.
Chain: every record, count and message of decode_batch_f32 against O.decode_frame_f32 (helpers.check_frame), the down-converter's
fractional frames included.  Subtraction: ft8rx_subtract_f32 against the oracle's double-precision subtraction on the same float
frames.  Reports: k_report under power-of-two scaling of its spectrum, and through the float chain."""
import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import float_frames_cases as F
import oracle as O
import report_cases as RC
import subtract_cases as SC
from helpers import check_frame
from pyft8_amd import _lib, ddc
from pyft8_amd.receiver import Receiver, config_from_kwargs
from test_gpu_parity import bits_equal
from test_gpu_subtract import BOUND, check_origins

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle(device=0, max_frames=8)
    yield h
    h.close()


@pytest.fixture(scope="module")
def ocfg():
    return O.default_config(**_lib.fft_plans())


# ---- 1. stages
@pytest.fixture(scope="module")
def stage(handle):
    """The stage batch through both float stage entries, once"""
    b = F.stage_batch()
    g, s = handle.spectrogram_f32(b), handle.cycle_spectrum_f32(b)
    g.setflags(write=False), s.setflags(write=False)
    return g, s


def test_stage_entries_equal_the_oracle(stage, ocfg):
    """[QUIET edge, LOUD edge, NORM edge, integer-valued test_08]: a loader that rounded, rescaled or truncated a sample, or a mask that
    let a neighbour's +-30000 c through, moves bits here"""
    g, s = stage
    for i, x in enumerate(F.stage_batch()):
        assert bits_equal(g[i], O.spectrogram_f32(x, ocfg)), i
        assert bits_equal(s[i].view(f32), O.cycle_spectrum_f32(x, ocfg).view(f32)), i
    assert np.isfinite(g).all() and g[:, 1:].min() > -239.9


def test_stage_entries_do_not_depend_on_the_neighbours(handle, stage):
    """The batch reversed: the frame behind the quiet one is no longer the loud one, and every frame's rows come out byte for byte"""
    g, s = stage
    rev = np.ascontiguousarray(F.stage_batch()[::-1])
    assert handle.spectrogram_f32(rev)[::-1].tobytes() == g.tobytes()
    assert handle.cycle_spectrum_f32(rev)[::-1].tobytes() == s.tobytes()


def test_stage_entries_equal_the_oracle_on_the_wide_build():
    cfg = config_from_kwargs(search_freq_range=[100, 4000])
    h = _lib.Handle(cfg, max_frames=1)
    try:
        assert h.wide and (h.grid_cols, h.spec_bins) == (1920, 96000)
        wcfg = O.default_config(sync_score_min=cfg.sync_score_min, max_cands=cfg.max_cands, f0_lo=cfg.f0_lo, f0_hi=cfg.f0_hi, h0_lo=cfg.h0_lo,
                                h0_hi=cfg.h0_hi)
        x = F.edge_frame("NORM")
        assert bits_equal(h.spectrogram_f32(x)[0], O.spectrogram_f32(x, wcfg))
        assert bits_equal(h.cycle_spectrum_f32(x)[0].view(f32), O.cycle_spectrum_f32(x, wcfg).view(f32))
    finally:
        h.close()


# ---- 2. chain
def test_chain_equals_the_oracle_on_level_and_down_converted_frames(handle, ocfg):
    """Eight frames in one batch: the six level frames and the two fractional frames the down-converter leaves in the float staging for
    the quiet stream -- records, counts, events and messages by the rule the int16 chain is held to"""
    q = F.quiet_stream()
    handle.ddc(q[None], ddc.IQ_F32, F.RATE, [0, 0], F.offsets(), d_f32_ptr=handle.staging_ptr_f32())
    y = handle.download_audio_f32(handle.staging_ptr_f32(), 2)
    assert 0.0 < np.abs(y).max() < 0.05 and ((y.view(np.uint32) & 0xFF) != 0).mean() > 0.9           # fractional, full mantissas
    frames = np.stack([x for _, _, x in F.level_frames()] + [y[0], y[1]])
    rec, cnt, ev, evc = handle.decode_batch_f32(frames)
    n = [check_frame(rec[i], cnt[i], ev[i], evc[i], frames[i], None, ocfg, decode=O.decode_frame_f32) for i in range(len(frames))]
    print(f"float chain against the oracle: messages per frame {n}")
    assert min(n[:6]) >= 20 and min(n[6:]) > 5


# ---- 3. subtraction
def _stage_and_subtract(h, frames, refine):
    h.decode_batch_f32(frames)                                                       # leaves the frames in the float staging
    res, orig = h.subtract(h.staging_ptr_f32(), len(frames), SC.signals(), refine=refine, return_float=True, return_origins=True,
                           float_frames=True)
    assert h.download_audio_f32(h.staging_ptr_f32(), len(frames)).tobytes() == res.tobytes()       # written back as it is
    return res, orig


@pytest.mark.parametrize("refine", [0, 2])
@pytest.mark.parametrize("level", ["NORM", "QUIET"])
def test_subtract_f32_matches_the_oracle(handle, level, refine):
    """SC.frames() * c through ft8rx_subtract_f32.  Origins: refine 0 leaves them as handed in; refine 2 against the oracle's picks on
    the int16 frames (the estimate does not depend on the level; none of the picks is a near tie).  Residual: the oracle subtracting
    at the GPU's own origins on the same float frames, max |gpu - oracle| <= 1e-4 of the scaled frame's RMS, all 6 x 180000 samples."""
    frames = F.scaled(SC.frames(), F.LEVELS[level])
    res, orig = _stage_and_subtract(handle, frames, refine)
    want = frames.copy()
    if refine == 2:
        picks, _ = SC.oracle_results(2)
        check_origins(orig, picks, 32)
        for f, sigs in enumerate(SC.signals()):
            for (tones, fHz0, tsec0), (fHz, tsec), (_, _, done) in zip(sigs, orig[f], picks[f]):
                assert O.refine2_subtract_at(want[f], tones, fHz0, tsec0, fHz, tsec) == done
    else:
        assert orig == [[(fHz, tsec) for _, fHz, tsec in sigs] for sigs in SC.signals()]
        for f, sigs in enumerate(SC.signals()):
            for tones, fHz, tsec in sigs:
                O.subtract(want[f], tones, fHz, tsec)
    assert np.abs(want[0] - frames[0]).max() > 100 * F.LEVELS[level]                 # something was subtracted
    rms = frames.astype(np.float64).std(axis=1)
    errs = np.abs(res.astype(np.float64) - want.astype(np.float64)).max(axis=1) / rms
    for f in range(len(frames)):
        print(f"float subtraction {level} refine {refine} frame {SC.NAMES[f]}: max|gpu - oracle| / rms = {errs[f]:.3e}  (rms {rms[f]:.3e})")
    assert (errs <= BOUND).all(), errs


@pytest.mark.parametrize("refine", [0, 2])
def test_subtract_f32_is_linear_under_a_power_of_two(handle, refine):
    """At c = 2^-15 the float residual is 2^-15 times the level-1 float residual, byte for byte: nothing between is not linear"""
    one = SC.frames().astype(f32)
    c = f32(2.0 ** -15)
    res1, orig1 = _stage_and_subtract(handle, one, refine)
    res, orig = _stage_and_subtract(handle, one * c, refine)
    assert orig == orig1
    assert res.tobytes() == (res1 * c).tobytes()
    assert np.abs(res1[0] - one[0]).max() > 100


# ---- 4. reports
@pytest.fixture(scope="module")
def report_base():
    h = _lib.Handle(max_frames=len(RC.spectra()))
    try:
        yield h, h.report_probe(RC.spectra(), *RC.columns(RC.cases()))
    finally:
        h.close()


@pytest.mark.parametrize("k", [-15, -30])
def test_report_probe_under_power_of_two_scaling(report_base, k):
    """k_report at the float path's levels: the spectra times 2^k give the flags, SNR, frequency and time of k = 0 byte for byte, and
    its score times 2^(2k) exactly, on every crafted case (the INVALID ones keep their NaNs)"""
    h, base = report_base
    got = h.report_probe(RC.spectra() * f32(2.0 ** k), *RC.columns(RC.cases()))
    assert (base["flags"] & _lib.RP_MEASURED).all() and np.isfinite(base["score"]).sum() >= 25
    for c, b, g in zip(RC.cases(), base, got):
        for key in ("flags", "snr_db", "f_hz", "t_sec", "pad"):
            assert g[key].tobytes() == b[key].tobytes(), (c[0], key, b, g)
        assert bits_equal(g["score"], b["score"] * f32(2.0 ** (2 * k))), (c[0], b, g)


def test_reports_through_the_float_chain():
    """decode_frames(float_frames=True) with reports on, on the integer frames times 2^-15, against the int16 chain: the messages are
    the same, and every message that comes from the same place in both runs (equal tsec, fHz and tweaks: the record's f0_idx, h0_idx,
    ttweak and ftweak) carries the same report.  The grid's log10f is not shifted exactly by the scaling, so a record may move: at
    most one message per frame may be left out for that (none moves in the oracle, tests/test_float_frames.py)."""
    a = F.int_frames()
    rx = Receiver("", None, reports=True, max_frames=4)
    try:
        want = rx.decode_frames(a)
        got = rx.decode_frames(a.astype(f32) * f32(2.0 ** -15), float_frames=True)
    finally:
        rx.close()
    same = left_out = 0
    for f in range(len(a)):
        assert [d["msg_tuple"] for d in got[f]] == [d["msg_tuple"] for d in want[f]], f
        out = 0
        for g, w in zip(got[f], want[f]):
            if (g["tsec"], g["fHz"], g["tweaks"]) != (w["tsec"], w["fHz"], w["tweaks"]):
                out += 1
                continue
            assert g["report"] == w["report"], (f, g, w)
            same += g["report"] is not None
        assert out <= 1, (f, out)
        left_out += out
    print(f"reports through the float chain: {same} compared, {left_out} left out for a record that moved")
    assert same >= 40
