"""ft8rx_subtract refine = 1 and refine = 2 (kernels/subtract.hpp: k_sub_scan, k_sub_pick, k_subd_mix, k_subd_model, k_subd_scan,
k_subd_accum, k_subd_apply) against the CPU oracle's double-precision statement of the same formulas, sample for sample, on the six
frames of tests/subtract_cases.py (13 signals: buffer edges, a signal that does not fit, neighbours, origins outside the buffer,
nothing to subtract) -- and the byte-for-byte invariances of refine 0, 1 and 2 (the sums of these kernels have a fixed order).

Origins: an arg-max on a grid, in float32 with hardware sin/cos on the GPU and in double in the oracle.  None of the oracle's 13 picks
is a near-tie (test_subtract_oracle.py::test_picks_are_stable_under_dither), so the GPU must pick the same grid point, with at most one
signal of the 13 one fine step off (the bound of test_multi_pass_matches_the_oracle_composition).
Residual: the oracle subtracts at exactly the origin the GPU returned (two doubles, the frequency a multiple of 1/64 Hz), so every
sample of every frame is compared even where an arg-max differs: max |gpu - oracle| <= 1e-4 of the RMS of the frame's int16 audio,
the figure every floating-point subtraction stage of this project is held to (measured values: profiles/subtract_notes.md)."""
import numpy as np
import pytest

import oracle as O
import subtract_cases as SC
from pyft8_amd import _lib

pytestmark = pytest.mark.gpu

B = len(SC.COUNTS)
BOUND = 1e-4                                                 # of the frame's RMS


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle(max_frames=B)
    yield h
    h.close()


def _subtract(h, refine, frames, sigs):
    """Stage the frames, subtract -> (float32 residual, origins, the int16 audio left on the device)."""
    frames = np.ascontiguousarray(frames)
    h.decode_batch(frames)                                   # leaves the frames in the handle's device staging buffer
    ptr = h.staging_ptr()
    res, orig = h.subtract(ptr, len(frames), sigs, refine=refine, return_float=True, return_origins=True)
    return res, orig, h.download_audio(ptr, len(frames))


_batch = {}


def batch(h, refine):
    """The one batch call over all six frames (counts 6, 4, 0, 1, 1, 1) of a mode, shared by the tests."""
    if refine not in _batch:
        res, orig, back = _subtract(h, refine, SC.frames(), SC.signals())
        for a in (res, back):
            a.setflags(write=False)
        _batch[refine] = (res, orig, back)
    return _batch[refine]


def check_origins(orig, picks, step):
    """Every origin within one fine step (`step` samples, 1/64 Hz) of the oracle's; at most one of the 13 off the oracle's point; the
    origins no shift could move exactly as they were handed in.  -> number off the oracle's point"""
    assert [len(o) for o in orig] == SC.COUNTS
    off = []
    for f in range(B):
        for i, (g, p) in enumerate(zip(orig[f], picks[f])):
            ds, dfq = SC.grid_delta(g, p)
            assert abs(ds) <= step and abs(dfq) <= 1.0 + 1e-6, (SC.NAMES[f], i, g, p)
            if ds != 0 or abs(dfq) > 1e-6:
                off.append((SC.NAMES[f], i, ds, dfq))
    assert orig[3] == [SC.O_ORIGINS[0]] and orig[4] == [SC.O_ORIGINS[1]]
    print(f"origins off the oracle's point: {len(off)} of {sum(SC.COUNTS)} {off}")
    assert len(off) <= 1, off
    return len(off)


def check_write_back(res, back):
    frames = SC.frames()
    for f in range(B):
        assert np.array_equal(back[f], O.to_int16(res[f])), SC.NAMES[f]
    for f in (2, 3, 4):                                      # nothing to subtract / no valid shift: the audio comes back as it went in
        assert np.array_equal(back[f], frames[f]), SC.NAMES[f]
        assert np.array_equal(res[f], frames[f].astype(np.float32)), SC.NAMES[f]


def check_residual(mode, res, want):
    errs = [float(np.abs(res[f].astype(np.float64) - want[f].astype(np.float64)).max()) / SC.rms(f) for f in range(B)]
    for f in range(B):
        print(f"refine {mode} frame {SC.NAMES[f]}: max|gpu - oracle| / rms = {errs[f]:.3e}  (rms {SC.rms(f):.1f})")
    assert all(e <= BOUND for e in errs), errs


def test_refine2_matches_the_oracle(handle):
    """refine = 2: origins against oracle.refine2_subtract; the residual against oracle.refine2_subtract_at applied signal by signal at
    the GPU's own origins (the decimated copy built around the origin handed in, as k_subd_mix builds it), all 6 x 180000 samples;
    the int16 audio left on the device is the rounded float residual."""
    res, orig, back = batch(handle, 2)
    picks, _ = SC.oracle_results(2)
    check_origins(orig, picks, 32)
    want = SC.frames().astype(np.float32)
    for f, sigs in enumerate(SC.signals()):
        for (tones, fHz0, tsec0), (fHz, tsec), (_, _, done) in zip(sigs, orig[f], picks[f]):
            assert O.refine2_subtract_at(want[f], tones, fHz0, tsec0, fHz, tsec) == done
    check_residual(2, res, want)
    check_write_back(res, back)


def test_refine1_matches_the_oracle(handle):
    """refine = 1: origins against oracle.refine1 (one full-rate fine step = 30 samples); the residual against oracle.subtract at the
    GPU's own origins -- the subtraction kernels are refine 0's, and so is the bound."""
    res, orig, back = batch(handle, 1)
    picks, _ = SC.oracle_results(1)
    check_origins(orig, picks, 30)
    want = SC.frames().astype(np.float32)
    for f, sigs in enumerate(SC.signals()):
        for (tones, _, _), (fHz, tsec), (_, _, done) in zip(sigs, orig[f], picks[f]):
            assert O.subtract(want[f], tones, fHz, tsec) == done
    check_residual(1, res, want)
    check_write_back(res, back)


def _same(got, want, rows=None):
    rows = range(len(want[0])) if rows is None else rows
    for k, f in enumerate(rows):
        assert got[0][k].tobytes() == want[0][f].tobytes() and got[2][k].tobytes() == want[2][f].tobytes(), SC.NAMES[f]
        assert got[1][k] == want[1][f], SC.NAMES[f]


@pytest.mark.parametrize("refine", [0, 1, 2])
def test_invariances(handle, refine):
    """Byte for byte (float residual, int16 audio, origins): a frame alone = its row of the batch; the batch reversed; a second run;
    max_sigs = 6 after max_sigs = 1 on a fresh handle (the signal table regrows) and the other way round; the (array, counts) fast
    path with junk in the rows at and beyond each frame's count, which are never read."""
    frames, sigs = SC.frames(), SC.signals()
    base = batch(handle, refine)
    _same(_subtract(handle, refine, frames, sigs), base)                                           # a second run
    for f in range(B):                                                                             # alone, B = 1, its own max_sigs
        _same(_subtract(handle, refine, frames[f:f + 1], [sigs[f]]), base, [f])
    rev = list(range(B))[::-1]
    _same(_subtract(handle, refine, frames[rev], [sigs[f] for f in rev]), base, rev)
    small = [2, 3, 4, 5]                                                                           # the frames with at most one signal
    h2 = _lib.Handle(max_frames=B)
    try:
        _same(_subtract(h2, refine, frames[small], [sigs[f] for f in small]), base, small)         # max_sigs = 1 first ...
        _same(_subtract(h2, refine, frames, sigs), base)                                           # ... then 6: the table regrows
    finally:
        h2.close()
    _same(_subtract(handle, refine, frames[small], [sigs[f] for f in small]), base, small)         # 1 after 6
    arr = np.zeros((B, max(SC.COUNTS)), _lib.SUBSIG_DTYPE)
    arr["fHz"], arr["tsec"], arr["tones"], arr["pad"] = np.nan, 1e9, 7, 0xA5
    for f in range(B):
        for i, (tones, fHz, tsec) in enumerate(sigs[f]):
            arr[f, i]["tones"], arr[f, i]["fHz"], arr[f, i]["tsec"] = tones, fHz, tsec
    handle.decode_batch(frames)
    ptr = handle.staging_ptr()
    res, orig = handle.subtract(ptr, B, (arr, np.array(SC.COUNTS, np.int32)), refine=refine, return_float=True, return_origins=True)
    _same((res, orig, handle.download_audio(ptr, B)), base)
