"""The noise blanker's numpy twin (pyft8_amd/blanker.py) on the crafted frames of tests/blanker_cases.py, the
taper against the library's (host only), the refusals, and what the blanker is for: on the impulse recipe the oracle gets back at least
half of the messages the impulses cost.  No GPU needed."""
import numpy as np
import pytest

import blanker_cases as cases
import oracle as O
from pyft8_amd import _lib, blanker

BLOCK = cases.BLOCK


def brute_weights(hit, guard, taper):
    """The gate by another route than the twin's scans: one shifted copy of the hit flags per distance, nearest first."""
    B, N = hit.shape
    H = guard + taper
    d = np.full((B, N), H + 1, np.int64)
    for o in range(H, -1, -1):
        d[:, o:][hit[:, :N - o]] = np.minimum(d[:, o:][hit[:, :N - o]], o)
        d[:, :N - o][hit[:, o:]] = np.minimum(d[:, :N - o][hit[:, o:]], o)
    T = [int(np.rint(32768.0 * 0.5 * (1.0 - np.cos(np.pi * j / (taper + 1.0))))) for j in range(1, taper + 1)]
    tab = np.array([0] * (guard + 1) + T + [32768], np.int64)
    return tab[d]


@pytest.mark.parametrize("k,guard,taper", cases.PARAM_SETS)
def test_twin_on_the_cases(k, guard, taper):
    q8 = int(np.rint(256 * k))
    bs, refs = cases.batches(k, guard, taper)
    names = [cases.ORDER[i:i + 3] for i in range(0, len(cases.ORDER), 3)]
    for x, (y, stats, lv), nm in zip(bs, refs, names):
        xs = x.astype(np.int64)
        a = np.abs(xs).reshape(3, 375, BLOCK)
        m = np.partition(a, 240, axis=2)[:, :, 240]
        assert np.array_equal(lv[:, :, 0], m)
        mp = np.pad(m, ((0, 0), (2, 2)), mode="edge")
        L = np.median(np.stack([mp[:, i:i + 375] for i in range(5)], axis=2), axis=2).astype(np.int64)
        assert np.array_equal(lv[:, :, 1], L)
        Ls = np.repeat(L, BLOCK, axis=1)
        hit = (Ls > 0) & (256 * np.abs(xs) > q8 * Ls)
        w = brute_weights(hit, guard, taper)
        assert np.array_equal(y[w == 32768], x[w == 32768])                                   # y = x wherever w = 32768
        assert np.array_equal(y, ((xs * w + 16384) >> 15).astype(np.int16))
        assert np.array_equal(stats, np.stack([hit.sum(1), (w < 32768).sum(1), (w == 0).sum(1), (L == 0).sum(1)], axis=1))
        for f in range(3):
            if stats[f, 0] == 0:
                assert y[f].tobytes() == x[f].tobytes(), nm[f]                                # a frame without hits keeps its bytes
            if nm[f] == "zeros":
                assert list(stats[f]) == [0, 0, 0, 375]
            if nm[f] == "early_pass":
                assert stats[f, 3] == 55 and lv[f, 319, 1] > 0 and lv[f, 320, 1] == 0
                assert not hit[f, 153600:].any() and hit[f, 153599]                           # L_b = 0: the planted samples there are no hits
            if nm[f] == "threshold":
                assert list(lv[f, 103:105, 1]) == [1024, 1024]
                assert [bool(hit[f, b * BLOCK + o]) for b in (103, 104) for o in (100, 300)] == [False, True, False, True]
                assert y[f, 103 * BLOCK + 100] == 4 * q8 and y[f, 103 * BLOCK + 300] == 0
            if nm[f] == "tied_medians":
                assert list(lv[f, 50:53, 0]) == [700, 500, 700] and lv[f, 200, 0] == 1234 and list(lv[f, 300:303, 0]) == [32768] * 3
            if nm[f] == "int16_min":
                assert hit[f, 4000] and y[f, 4000] == 0
            if nm[f] == "burst":
                assert hit[f, 250 * BLOCK + 120:250 * BLOCK + 360].all() and lv[f, 250, 0] > 10000 > lv[f, 250, 1]
            if nm[f] == "ends" and k == 8.0:
                H = guard + taper
                assert hit[f, [0, 1, H, cases.NSAMP - 1 - H, cases.NSAMP - 1]].all() and stats[f, 0] == len({0, 1, H}) + len({cases.NSAMP - 1 - H, cases.NSAMP - 1})
    # the first batch: a hit in the last sample of frame 0 touches nothing at the start of frame 1
    x, (y, stats, _) = bs[0], refs[0]
    assert y[0, -1] == 0 and y[1, :40 - min(guard + taper, 40)].tobytes() == x[1, :40 - min(guard + taper, 40)].tobytes()
    if k == 8.0:
        assert y[1, :400].tobytes() == x[1, :400].tobytes()
    # one frame alone is the same as inside a batch
    for f in (1, 2):
        y1, s1, l1 = blanker.reference(x[f], k, guard, taper)
        assert y1.tobytes() == y[f].tobytes() and np.array_equal(s1[0], stats[f]) and np.array_equal(l1[0], refs[0][2][f])


def test_taper_is_the_librarys():
    for R in range(65):
        assert np.array_equal(blanker.taper_table(R), _lib.blank_taper(R)), R
    assert list(blanker.taper_table(1)) == [16384] and len(_lib.blank_taper(0)) == 0
    t = blanker.taper_table(64)
    assert (np.diff(t) > 0).all() and 0 < t[0] and t[-1] < 32768
    L = _lib.lib()
    assert L.ft8rx_blank_taper(65, None, 0) == -1 and L.ft8rx_blank_taper(-1, None, 0) == -1 and L.ft8rx_blank_taper(6, None, 0) == 6


def test_parameters_and_refusals_by_name():
    assert blanker.params(None) is None and blanker.params(False) is None
    assert blanker.params(True) == (2048, 6, 6) == blanker.check()
    assert blanker.params(5.5) == (1408, 6, 6) and blanker.params(2) == (512, 6, 6) and blanker.params(64) == (16384, 6, 6)
    assert blanker.params({"threshold": 7, "guard": 0, "taper": 64}) == (1792, 0, 64)
    assert blanker.params({"guard": 64}) == (2048, 64, 6)
    x = np.zeros((1, cases.NSAMP), np.int16)
    for kw, name in (({"threshold": 1.99}, "threshold"), ({"threshold": 64.01}, "threshold"), ({"threshold": float("nan")}, "threshold"),
                     ({"guard": 65}, "guard"), ({"guard": -1}, "guard"), ({"guard": 2.5}, "guard"), ({"taper": -1}, "taper"),
                     ({"taper": 65}, "taper")):
        with pytest.raises(_lib.Ft8rxError, match=name + "="):
            blanker.params(kw)
        with pytest.raises(_lib.Ft8rxError, match=name + "="):
            blanker.reference(x, **kw)
    with pytest.raises(_lib.Ft8rxError, match="gaurd"):
        blanker.params({"gaurd": 3})
    with pytest.raises(_lib.Ft8rxError, match="noise_blanker="):
        blanker.params("on")
    with pytest.raises(_lib.Ft8rxError, match="180000"):
        blanker.reference(np.zeros((2, 1000), np.int16))


def test_impulse_recipe_is_seeded_and_clipped():
    clean, noisy, _ = cases.recipe()
    again = blanker.add_impulses(clean[0], np.random.default_rng(cases.RECIPE_SEED), cases.RECIPE_RATE, cases.RECIPE_PEAK)
    assert again.tobytes() == noisy[0].tobytes() and noisy.dtype == np.int16
    changed = (noisy != clean).sum(axis=1)
    assert (changed > 5000).all() and (changed < 9000).all()                  # ~1500 impulses of 5 samples per frame
    assert np.abs(noisy.astype(np.int64)).max() >= 32767                      # peaks up to 45 sigma: some are clipped


def test_benefit_on_the_impulse_recipe():
    """The oracle's true decodes on the three recipe frames: clean C, with impulses N, after the twin's blanking K.  The recipe must hurt
    (N <= C - 12), the blanker must recover at least half of what was lost, with no more false decodes than the clean frames have.
    Measured: C, N, K = 68, 24, 62 with 2, 1, 0 false decodes."""
    clean, noisy, truth = cases.recipe()
    blanked, stats, _ = blanker.reference(noisy)
    ocfg = O.default_config(**_lib.fft_plans())

    def count(frames):
        good = bad = 0
        for f, t in zip(frames, truth):
            texts = [" ".join(m["msg_tuple"]) for m in O.decode_frame(f, ocfg)["msgs"]]
            good += sum(x in t for x in texts)
            bad += sum(x not in t for x in texts)
        return good, bad
    (C, fc), (N, fn), (K, fk) = count(clean), count(noisy), count(blanked)
    print(f"benefit: C, N, K = {C}, {N}, {K}; false {fc}, {fn}, {fk}; hits per frame {list(stats[:, 0])}")
    assert N <= C - 12
    assert K >= N + (C - N) / 2
    assert fk <= fc
    assert (blanker.reference(clean)[1][:, 0] == 0).all()                     # k = 8 never hits on the clean frames
