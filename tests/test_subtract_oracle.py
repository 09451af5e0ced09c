"""The CPU oracle's statements of ft8rx_subtract refine = 1 and refine = 2 (oracle/ft8_oracle.c: ft8o_refine1, ft8o_refine2_subtract,
ft8o_refine2_subtract_at) on the frames of tests/subtract_cases.py: what tests/test_gpu_subtract.py compares the kernels with must
itself be right -- against truth, against its own earlier version, and not sitting on a near-tie."""
import os

import numpy as np
import pytest

import oracle as O
import subtract_cases as SC
from conftest import GOLDEN

FITS = [(f, i) for f in (0, 1) for i in range(SC.COUNTS[f]) if (f, i) != (0, SC.E_UNFIT)] + [(5, 0)]


def test_refine2_refactor_is_byte_identical():
    """ft8o_refine2_subtract, now the scans followed by the shared subtraction of ft8o_refine2_subtract_at, against what commit 376f6fd
    (one function, before the split) returned on the edge frame: tests/golden/subtract_edge_refine2.npz, made by
    oracle/gen_golden_subtract_edge.py with that commit's oracle.  Origins and every sample of the residual, bit for bit."""
    g = np.load(os.path.join(GOLDEN, "subtract_edge_refine2.npz"))
    picks, resid = SC.oracle_results(2)
    assert [(f, t) for f, t, _ in picks[0]] == [tuple(o) for o in g["origins"].tolist()]
    assert [d for _, _, d in picks[0]] == [bool(d) for d in g["done"]]
    assert resid[0].tobytes() == g["residual"].tobytes()


def test_refine2_subtract_at_its_own_origin_is_refine2_subtract():
    """Handed the origin refine2_subtract picked, refine2_subtract_at leaves the same bytes -- signal by signal on the running residual,
    all six frames."""
    picks, resid = SC.oracle_results(2)
    wf = SC.frames().astype(np.float32)
    for f, sigs in enumerate(SC.signals()):
        for (tones, fHz0, tsec0), (fHz, tsec, done) in zip(sigs, picks[f]):
            assert O.refine2_subtract_at(wf[f], tones, fHz0, tsec0, fHz, tsec) == done, (f, fHz, tsec)
        assert wf[f].tobytes() == resid[f].tobytes(), SC.NAMES[f]


@pytest.mark.parametrize("mode", [1, 2])
def test_refined_origins_hit_the_truth(mode):
    """Every signal that fits the buffer lands within 3 ms and 0.1 Hz of where it was put (the window of
    test_multi_pass_decode_with_subtraction) and is subtracted; the one that runs off the end locks where the whole model still fits."""
    picks, _ = SC.oracle_results(mode)
    truth = SC.truth()
    for f, i in FITS:
        (fHz, tsec, done), (f0, t0) = picks[f][i], truth[f][i]
        assert done and abs(tsec - t0) < 0.003 and abs(fHz - f0) < 0.1, (mode, f, i, fHz - f0, tsec - t0)
    fHz, tsec, done = picks[0][SC.E_UNFIT]
    s0 = int(12000.0 * tsec)
    assert done and 0 < s0 <= SC.NSAMP - SC.SUB_L < int(12000.0 * truth[0][SC.E_UNFIT][1]), (mode, fHz, tsec)
    if mode == 1:                                            # the two time grids differ (30 samples against 32): printed, not asserted
        p2, _ = SC.oracle_results(2)
        for f in range(len(SC.COUNTS)):
            for i, (a, b) in enumerate(zip(picks[f], p2[f])):
                ds, dfq = SC.grid_delta(a, b)
                print(f"refine 1 - refine 2, {SC.NAMES[f]}[{i}]: {ds:+d} samples, {dfq:+.0f}/64 Hz")


@pytest.mark.parametrize("mode", [1, 2])
def test_origins_outside_the_buffer(mode):
    """tsec = -0.5 and 20.0: no shift is valid, origin and audio stay as they are.  tsec = 0.0 (start sample 0, itself invalid): the
    positive shifts are valid, the origin moves onto the signal and it is subtracted."""
    picks, resid = SC.oracle_results(mode)
    frames = SC.frames()
    for f in (3, 4):
        assert picks[f] == [SC.O_ORIGINS[f - 3] + (False,)]
        assert np.array_equal(resid[f], frames[f].astype(np.float32))
    assert np.array_equal(resid[2], frames[2].astype(np.float32))                   # frame Z
    # refine 2: the only valid coarse shift is +128 and the fine scan stays on it; refine 1: coarse +120, fine 0
    assert picks[5] == [(1002.75, ((128.5 if mode == 2 else 120.5)) / 12000.0, True)]
    assert not np.array_equal(resid[5], frames[5].astype(np.float32))


@pytest.mark.parametrize("mode", [1, 2])
def test_picks_are_stable_under_dither(mode):
    """The GPU test asks for the oracle's own grid point: that is only fair where the arg-max is no near-tie.  A +-0.01-count dither of
    the input (100 x the float32 rounding of a sample, 1e-5 of the noise) moves none of the 13 picks of either oracle."""
    picks, _ = SC.oracle_results(mode)
    for seed in (11, 12):
        rng = np.random.default_rng(seed)
        wf = (SC.frames().astype(np.float64) + rng.uniform(-0.01, 0.01, SC.frames().shape)).astype(np.float32)
        for f, sigs in enumerate(SC.signals()):
            got = SC.run_oracle(mode, wf[f], sigs)
            assert got == picks[f], (mode, seed, SC.NAMES[f], got, picks[f])
