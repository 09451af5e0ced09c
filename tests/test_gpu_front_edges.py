"""The front-end kernels on designed inputs (tests/front_cases.py): grids of small integers, on which every score is exact and equal
scores are everywhere, and spectra of a few bins, on which every metric of the fine sync is a tie or an exact zero.  Every comparison
is with the CPU oracle (or the numpy twins of weak mode and FT4) and is exact: integers as they are, floats bit for bit, NaNs by
position.  What the fixtures hold is asserted without a GPU in tests/test_front_cases.py; what is compared here:

  k_sync / k_sync3     `score > best` inside a thread row, the lowest h0 among equal maxima of the 16 thread rows
  k_sync_acc / _acc3   a later window of a wide time range replaces the stored result only if strictly larger (alias rows 750 later)
  k_topk               the strict threshold, f0 order among equal scores, the cut at max_cands inside a run of equal scores, 2048 keys
  k_ft4_sync / _peaks  the fp64 ties, the inclusive threshold, "a tie goes to the lower bin"
  k_grid_llr           the snr's truncation and clamp, sd = 0, rows outside 1 .. 375 after the modulo-750 wrap, exact-zero LLRs
  k_fine / _td / _weak the arg-max choices when every metric is equal, structurally zero inputs of the first FFT stage"""
import numpy as np
import pytest

import front_cases as F
import oracle as O
import weak_twin as W
from helpers import bits_equal
from pyft8_amd import _lib, ft4

pytestmark = pytest.mark.gpu

CFG = O.default_config()
DEFAULT = (CFG.f0_lo, CFG.f0_hi, CFG.h0_lo, CFG.h0_hi)
FULL = (CFG.f0_lo, CFG.f0_hi) + F.FULL_H0
FT4_RANGE = ft4.freq_range_to_f0() + ft4.time_range_to_h0()
WIDE_F0_HI = 1800
BATCH = 4                                                         # grids per call
MAX_FRAMES = 6                                                    # ... and spectra per call: every handle's max_frames


@pytest.fixture(scope="module")
def handles():
    """one handle per configuration, made on first use, closed with the module"""
    made = {}

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in made:
            made[key] = _lib.Handle(_lib.default_config(**kw), max_frames=MAX_FRAMES)
        return made[key]
    yield get
    for h in made.values():
        h.close()


def search_grids():
    return [("quantised", F.quantised_grid()), ("coarse", F.coarse_grid()), ("periodic", F.periodic_grid()),
            ("flat 0.0", F.flat_grid(0.0)), ("flat 1.0", F.flat_grid(1.0))]


def check_search(h, grids, okw):
    """Handle.sync_search on named grids (batches of BATCH) against O.sync_search with the same settings -> {name: [f0 of the list]}"""
    out = {}
    for lo in range(0, len(grids), BATCH):
        part = grids[lo:lo + BATCH]
        f0, h0, sc, cnt = h.sync_search(np.stack([g for _, g in part]))
        for i, (name, g) in enumerate(part):
            want = O.sync_search(g, O.default_config(**okw))
            n = int(cnt[i])
            assert n == len(want), (name, n, len(want))
            assert list(f0[i, :n]) == [c.f0_idx for c in want], name
            assert list(h0[i, :n]) == [c.h0_idx for c in want], name
            assert bits_equal(sc[i, :n], np.array([c.score for c in want], np.float32)), name
            out[name] = [int(v) for v in f0[i, :n]]
    return out


@pytest.mark.parametrize("max_cands", [4, 200, 928])
def test_search_default_window(handles, max_cands):
    """count, f0, h0 and score bits of the candidate lists; at 4 and 200 the cut falls inside a run of equal scores on the quantised,
    the coarse and the periodic grid (the run's members are kept in f0 order), 928 takes every column; the flat grids give nothing"""
    got = check_search(handles(max_cands=max_cands, sync_score_min=0.0), search_grids(), dict(max_cands=max_cands, sync_score_min=0.0))
    assert len(got["quantised"]) == len(got["coarse"]) == len(got["periodic"]) == max_cands
    assert got["flat 0.0"] == got["flat 1.0"] == []


def test_search_threshold_is_strict(handles):
    """sync_score_min = t, a score that several columns attain exactly: they are left out; nextafter(t, -inf): they are taken"""
    g = F.quantised_grid()
    t = np.float32(F.attained_threshold(g, *DEFAULT))
    below = np.nextafter(t, np.float32(-np.inf))
    best, _ = F.best_of_map(F.score_map(g, *DEFAULT), DEFAULT[2])
    at_t = {DEFAULT[0] + int(i) for i in np.nonzero(best == t)[0]}
    assert len(at_t) >= 2
    grids = search_grids()[:BATCH]
    out = check_search(handles(max_cands=928, sync_score_min=float(t)), grids, dict(max_cands=928, sync_score_min=float(t)))
    take = check_search(handles(max_cands=928, sync_score_min=float(below)), grids, dict(max_cands=928, sync_score_min=float(below)))
    assert not at_t & set(out["quantised"]) and at_t <= set(take["quantised"])
    assert len(take["quantised"]) == len(out["quantised"]) + len(at_t)


@pytest.mark.parametrize("f0_range", [(4, 961), (33, 50), (960, 961)])
def test_per_column_results(handles, f0_range):
    """Handle.sync_scores over the legal ends, a tile with one live lane and the last column alone (its tones reach column 973) against
    the oracle's per-column result; a column the oracle omits is (0.0, h0 0)"""
    h = handles(max_cands=200, sync_score_min=0.0)
    grids = search_grids()[:BATCH]
    sc, h0 = h.sync_scores(np.stack([g for _, g in grids]), *f0_range)
    for i, (name, g) in enumerate(grids):
        w_sc, w_h0 = F.oracle_columns(g, {}, *f0_range)
        assert bits_equal(sc[i], w_sc) and np.array_equal(h0[i], w_h0), (name, f0_range)
    assert (sc[3] == 0).all() and (h0[3] == 0).all()              # the flat grid


def test_window_seams(handles):
    """h0 range (-898, 578): k_sync and four k_sync_acc launches.  In 900 or so columns the winner's alias 750 rows later lies in a
    later launch with the same rows and so the same score: the earlier h0 must survive"""
    okw = dict(h0_lo=FULL[2], h0_hi=FULL[3], max_cands=200, sync_score_min=0.0)
    h = handles(**okw)
    g = F.quantised_grid()
    S = F.score_map(g, *FULL)
    best, first = F.best_of_map(S, FULL[2])
    k = first - FULL[2]
    cols = np.arange(S.shape[1])
    alias = (k + 750 < S.shape[0]) & (best > 0)
    alias[alias] = S[k[alias] + 750, cols[alias]] == best[alias]
    assert alias.sum() >= 500
    grids = [("quantised", g), ("coarse", F.coarse_grid()), ("periodic", F.periodic_grid())]
    sc, h0 = h.sync_scores(np.stack([x for _, x in grids]), FULL[0], FULL[1])
    for i, (name, x) in enumerate(grids):
        w_sc, w_h0 = F.oracle_columns(x, dict(h0_lo=FULL[2], h0_hi=FULL[3]), FULL[0], FULL[1])
        assert bits_equal(sc[i], w_sc) and np.array_equal(h0[i], w_h0), name
    assert np.array_equal(h0[0][alias], first[alias]) and (h0[0][alias] + 750 < FULL[3]).all()
    check_search(h, grids, okw)


def test_weak_mode_scores(handles):
    """k_sync3 on the default range, k_sync3 and eleven k_sync3_acc launches on (-898, 578), against the twin's three-block score"""
    grids = [("quantised", F.quantised_grid()), ("coarse", F.coarse_grid()), ("periodic", F.periodic_grid())]
    stack = np.stack([g for _, g in grids])
    sc, h0 = handles(max_cands=200, sync_score_min=0.0).sync_scores(stack, DEFAULT[0], DEFAULT[1], weak=True)
    for i, (name, g) in enumerate(grids):
        w_sc, w_h0 = W.sync3_scores(g, *DEFAULT)
        assert bits_equal(sc[i], w_sc) and np.array_equal(h0[i], w_h0), name
    rng = (32, 96) + F.FULL_H0                                    # four tiles of the full time range
    sc, h0 = handles(h0_lo=FULL[2], h0_hi=FULL[3], max_cands=200, sync_score_min=0.0).sync_scores(stack, rng[0], rng[1], weak=True)
    for i, (name, g) in enumerate(grids):
        w_sc, w_h0 = W.sync3_scores(g, *rng)
        assert bits_equal(sc[i], w_sc) and np.array_equal(h0[i], w_h0), name
        if name == "quantised":
            _, first, _, n_alias = F.weak_census(g, *rng)
            assert n_alias >= 32 and np.array_equal(h0[i], first)


@pytest.mark.parametrize("max_cands", [4, WIDE_F0_HI - 32])
def test_search_wide_build(handles, max_cands):
    """the wide library (f0_hi = 1800): 1768 columns, 2048 keys in k_topk, two per thread"""
    h = handles(f0_hi=WIDE_F0_HI, max_cands=max_cands, sync_score_min=0.0)
    assert h.wide
    g = F.quantised_grid(wide=True)
    f0, h0, sc, cnt = h.sync_search(g)
    want = O.sync_search(g, O.default_config(f0_hi=WIDE_F0_HI, max_cands=max_cands, sync_score_min=0.0))
    n = int(cnt[0])
    assert n == len(want) == max_cands
    assert list(f0[0, :n]) == [c.f0_idx for c in want] and list(h0[0, :n]) == [c.h0_idx for c in want]
    assert bits_equal(sc[0, :n], np.array([c.score for c in want], np.float32))


@pytest.mark.parametrize("max_cands", [4, 256])
def test_ft4_search(handles, max_cands):
    """Handle.ft4_sync on the multiples-of-3 grid against ft4.search: the list, the per-bin best scores (float32 of exact integers) and
    the per-bin best h0, all exactly equal -- at a threshold below every maximum, at an attained integer t (kept: the threshold is
    inclusive) and at t + 1, on the default range (rows outside the grid are read) and on one of 37 bins"""
    h = handles(max_cands=max_cands, sync_score_min=0.0)
    db = F.ft4_grid()
    t = F.ft4_attained_threshold(db, *FT4_RANGE)
    n_at = {}
    try:
        for rng, sync_min in [(FT4_RANGE, F.FT4_SYNC_MIN), (FT4_RANGE, t), (FT4_RANGE, t + 1.0),
                              (F.FT4_NARROW + FT4_RANGE[2:], F.FT4_SYNC_MIN), (F.FT4_NARROW + FT4_RANGE[2:], t)]:
            h.ft4_set(sync_min=sync_min)
            h.ft4_set_range(*rng)
            f0, h0, sc, cnt, bs, bh = h.ft4_sync(db, want_best=True)
            want, best, w_bh, _ = ft4.search(db, *rng, sync_min=sync_min, max_cands=max_cands, full=True)
            n = int(cnt[0])
            assert n == len(want), (rng, sync_min, n, len(want))
            assert [(int(a), int(b)) for a, b in zip(f0[0, :n], h0[0, :n])] == [(c[0], c[1]) for c in want], (rng, sync_min)
            assert np.array_equal(sc[0, :n], np.array([c[2] for c in want], np.float32)), (rng, sync_min)
            assert (best == np.rint(best)).all() and np.array_equal(bs[0], best.astype(np.float32)), (rng, sync_min)
            assert np.array_equal(bh[0], w_bh), (rng, sync_min)
            if rng == FT4_RANGE:
                n_at[sync_min] = int((sc[0, :n] == np.float32(t)).sum())
    finally:
        h.ft4_set_range()
        h.ft4_set()
    if max_cands == 256:                                          # nothing is cut: the candidates at t are there at t, gone at t + 1
        assert n_at[t] >= 2 and n_at[t + 1.0] == 0


@pytest.mark.parametrize("n", [1, 65, 300])
def test_grid_llrs(handles, n):
    """Handle.llr_grid on the LLR grid and the three designed search grids against O.db_to_llr(O.payload(...)): LLR bits, sd bits, snr"""
    h = handles(max_cands=200, sync_score_min=0.0)
    grids = [F.llr_grid(), F.quantised_grid(), F.coarse_grid(), F.periodic_grid()]
    trip = F.llr_triples(len(grids), n)
    llr, sd, snr = h.llr_grid(np.stack(grids), *[np.array([t[k] for t in trip], np.int32) for k in range(3)])
    want = {}
    for i, (fr, f0, h0) in enumerate(trip):
        if (fr, f0, h0) not in want:
            want[(fr, f0, h0)] = O.db_to_llr(O.payload(grids[fr], f0, h0))
        w_llr, w_sd, w_snr, _ = want[(fr, f0, h0)]
        assert bits_equal(llr[i], w_llr) and bits_equal(sd[i:i + 1], np.float32([w_sd])) and snr[i] == w_snr, (fr, f0, h0)
    if n == 300:
        # every designed span is there with its snr; the flat payload: sd 0, 174 NaNs, snr -24; the aliases of h0 -37 are byte-identical
        where = {t: i for i, t in enumerate(trip)}
        for (span, w_snr), f0 in zip(F.LLR_SPANS, F.LLR_F0):
            assert snr[where[(0, f0, F.LLR_H0)]] == w_snr, span
        i = where[(0,) + F.LLR_FLAT]
        assert np.isnan(llr[i]).all() and sd[i] == 0 and snr[i] == -24
        assert (llr[where[(1, 4, 86)]] == 0).any()                # ties among the eight tones: exact zeros
        for fr in range(len(grids)):
            for f0 in F.LLR_EDGE_F0:
                a = where[(fr, f0, -37)]
                for h0 in (713, -787):
                    b = where[(fr, f0, h0)]
                    assert llr[a].tobytes() == llr[b].tobytes() and sd[a].tobytes() == sd[b].tobytes() and snr[a] == snr[b], (fr, f0, h0)


def _fine_equal(r, k, w, key):
    assert (r["ret"][k], r["ttweak"][k], r["ftweak"][k], r["nsync"][k]) == (w["ret"], w["ttweak"], w["ftweak"], w["nsync"]), key
    assert bits_equal(r["sgrid"][k], w["sgrid"]), key
    if w["ret"] != 0:
        assert bits_equal(r["llr"][k], w["llr"]) and bits_equal(r["sd"][k:k + 1], np.float32([w["sd"]])) and r["snr"][k] == w["snr"], key


def test_fine_sync(handles):
    """Handle.fine on the designed spectra for f0 at both ends and h0 on both sides of the frequency-domain range (k_fine and
    k_fine_td) against O.fine under the library's plans; the all-zero spectrum resolves every tie to the first trial of either scan"""
    h = handles(max_cands=200, sync_score_min=0.0)
    ocfg = W.oracle_config()
    spec, trip = F.spectra(), F.fine_triples()
    r = h.fine(spec, *[np.array([t[k] for t in trip], np.int32) for k in range(3)], want_sgrid=True)
    tweaks = set()
    for k, (fr, f0, h0) in enumerate(trip):
        w = O.fine(spec[fr], f0, h0, ocfg)
        _fine_equal(r, k, w, (F.SPECTRA[fr], f0, h0))
        tweaks.add((w["ttweak"], w["ftweak"]))
        if fr == 0:
            assert (r["ret"][k], r["ttweak"][k], r["ftweak"][k], r["nsync"][k]) == (0, -8, -32, 3) and (r["sgrid"][k] == 0).all()
    assert len(tweaks) >= 6, tweaks                               # the other spectra give other, non-trivial tweaks


def test_fine_sync_weak(handles):
    """the same spectra and triples through k_fine_weak against the twin's joint scan"""
    h = handles(max_cands=200, sync_score_min=0.0)
    spec = F.spectra()
    trip = [t for t in F.fine_triples() if t[2] not in (-140, 220)]       # (the two sides of k_fine's range are one kernel here)
    r = h.fine(spec, *[np.array([t[k] for t in trip], np.int32) for k in range(3)], want_sgrid=True, weak=True)
    want = W.fine_weak_many(spec, trip, W.oracle_config())
    for k, (fr, f0, h0) in enumerate(trip):
        _fine_equal(r, k, want[k], (F.SPECTRA[fr], f0, h0))
