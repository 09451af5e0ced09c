"""The designed front-end fixtures (tests/front_cases.py) really hold the cases they are there for -- asserted without a GPU, on numpy,
the oracle and the twins alone.  These are conditions on the fixtures, not measurements of the library; tests/test_gpu_front_edges.py
runs the kernels on the same fixtures."""
import numpy as np
import pytest

import front_cases as F
import oracle as O
import weak_twin as W
from helpers import bits_equal
from pyft8_amd import ft4

CFG = O.default_config()
DEFAULT = (CFG.f0_lo, CFG.f0_hi, CFG.h0_lo, CFG.h0_hi)          # 928 columns, h0 -37 .. 86: one k_sync launch
FULL = (CFG.f0_lo, CFG.f0_hi) + F.FULL_H0                       # h0 -898 .. 577: k_sync and four k_sync_acc launches
FT4_RANGE = ft4.freq_range_to_f0() + ft4.time_range_to_h0()     # (2, 567, -42, 168): rows outside the grid are read


def _map_is_the_oracle(grid, rng, cfg_kw):
    best, bh = F.best_of_map(F.score_map(grid, *rng), rng[2])
    o_best, o_bh = F.oracle_columns(grid, cfg_kw, rng[0], rng[1])
    return bits_equal(best, o_best) and np.array_equal(bh, o_bh)


@pytest.mark.parametrize("name", ["quantised", "coarse", "periodic"])
def test_score_map_is_the_oracle_search(name):
    """the census counts ties on a numpy score map: its first strict maxima are the oracle's, bit for bit, on every designed grid"""
    grid = {"quantised": F.quantised_grid, "coarse": F.coarse_grid, "periodic": F.periodic_grid}[name]()
    assert _map_is_the_oracle(grid, DEFAULT, {})
    if name == "quantised":
        assert _map_is_the_oracle(grid, FULL, dict(h0_lo=FULL[2], h0_hi=FULL[3]))
        wide = F.quantised_grid(wide=True)
        assert wide.shape == (F.ROWS, F.COLS_WIDE) and _map_is_the_oracle(wide, (32, 1800) + DEFAULT[2:], {})


def test_cells_are_small_integers():
    for g in (F.quantised_grid(), F.quantised_grid(wide=True), F.coarse_grid(), F.periodic_grid(), F.ft4_grid()):
        assert np.array_equal(g, np.rint(g)) and g.min() >= 0 and g.max() < 64
    for g in (F.quantised_grid(), F.quantised_grid(wide=True), F.ft4_grid()):
        assert np.array_equal(np.unique(g), 3.0 * np.arange(12))
    assert np.array_equal(np.unique(F.coarse_grid()), [0.0, 30.0])
    assert np.array_equal(F.periodic_grid()[16:], F.periodic_grid()[:-16])


def test_quantised_grid_holds_the_ties():
    g = F.quantised_grid()
    t = F.attained_threshold(g, *DEFAULT)
    c = F.search_census(g, *DEFAULT, max_cands=(4, 200, 928), thresholds=(t,))
    assert c["columns"] == 928 and c["distinct"] < 200
    assert c["h0_tied"] >= 10 and c["lower_row"] >= 5
    assert c["groups"] >= 100
    # the cut falls inside a run of equal scores at every max_cands below the number of columns; 928 takes every column
    assert c["cut"][4] is not None and 0 < c["cut"][4][0] < c["cut"][4][1]
    assert c["cut"][200] is not None and 0 < c["cut"][200][0] < c["cut"][200][1]
    assert c["cut"][928] is None
    assert c["attained"][t] >= 2
    assert np.nextafter(np.float32(t), np.float32(-np.inf)) < np.float32(t)


def test_coarse_grid_holds_many_more_ties():
    g = F.coarse_grid()
    t = F.attained_threshold(g, *DEFAULT)
    c = F.search_census(g, *DEFAULT, max_cands=(4, 200), thresholds=(t,))
    assert c["h0_tied"] >= 100 and c["lower_row"] >= 50 and c["same_row"] >= 5
    assert c["cut"][4] is not None and c["cut"][200] is not None and c["attained"][t] >= 2


def test_periodic_grid_ties_meet_inside_one_thread_row():
    g = F.periodic_grid()
    t = F.attained_threshold(g, *DEFAULT)
    c = F.search_census(g, *DEFAULT, max_cands=(4, 200), thresholds=(t,))
    assert c["columns"] == c["h0_tied"] == c["same_row"] == 928 and c["lower_row"] == 0
    assert c["cut"][4] is not None and c["cut"][200] is not None and c["attained"][t] >= 2


def test_flat_grids_yield_nothing():
    assert (F.score_map(F.flat_grid(0.0), *DEFAULT) == 0).all()
    assert (F.score_map(F.flat_grid(1.0), *DEFAULT) == np.float32(14.0 + F.W6 * 84.0)).all() and 14.0 + F.W6 * 84.0 < 0
    for v in (0.0, 1.0):
        assert O.sync_search(F.flat_grid(v), O.default_config(sync_score_min=0.0, max_cands=2048)) == []


def test_full_range_holds_the_alias_ties():
    c = F.search_census(F.quantised_grid(), *FULL, max_cands=(200,))
    assert c["alias"] >= 500 and c["cut"][200] is not None


def test_wide_grid_holds_the_ties():
    c = F.search_census(F.quantised_grid(wide=True), 32, 1800, *DEFAULT[2:], max_cands=(4, 1768))
    assert c["columns"] == 1768 > 1024                           # beyond the default build's keys: two per thread in k_topk
    assert c["h0_tied"] >= 10 and c["lower_row"] >= 5 and c["groups"] >= 100
    assert c["cut"][4] is not None and c["cut"][1768] is None


def test_weak_score_holds_the_ties():
    g = F.quantised_grid()
    best, bh, tied, _ = F.weak_census(g, *DEFAULT)
    t_best, t_bh = W.sync3_scores(g, *DEFAULT)
    assert bits_equal(best, t_best) and np.array_equal(bh, t_bh)
    assert tied >= 5
    best, bh, tied, alias = F.weak_census(g, 32, 96, *F.FULL_H0)            # 64 columns of the full range: k_sync3_acc across aliases
    t_best, t_bh = W.sync3_scores(g, 32, 96, *F.FULL_H0)
    assert bits_equal(best, t_best) and np.array_equal(bh, t_bh)
    assert alias >= 32


def test_ft4_grid_holds_the_ties():
    db = F.ft4_grid()
    t = F.ft4_attained_threshold(db, *FT4_RANGE)
    assert t == np.rint(t) and t > 0
    c = F.ft4_census(db, *FT4_RANGE, sync_min=F.FT4_SYNC_MIN)
    assert c["integer"]
    assert c["plateaus"] >= 5 and c["plateau_peaks"] >= 1 and c["h0_tied"] >= 5 and c["lower_row"] >= 3 and c["shared"] >= 50
    assert F.ft4_census(db, *FT4_RANGE, sync_min=t)["attained"] >= 2
    # the inclusive threshold: the candidates at t are kept at sync_min = t and gone at t + 1
    at_t = [x for x in ft4.search(db, *FT4_RANGE, sync_min=t, max_cands=2048) if x[2] == t]
    assert len(at_t) >= 2 and all(x[2] > t for x in ft4.search(db, *FT4_RANGE, sync_min=t + 1, max_cands=2048))
    # a range that is no multiple of the kernel's 16-bin tile still has candidates
    assert (F.FT4_NARROW[1] - F.FT4_NARROW[0]) % 16 != 0
    assert len(ft4.search(db, *F.FT4_NARROW, *FT4_RANGE[2:], sync_min=F.FT4_SYNC_MIN, max_cands=2048)) >= 5


def test_llr_grid_holds_the_edges():
    c = F.llr_census(F.llr_grid())
    assert c["spans"] == {span: snr for span, snr in F.LLR_SPANS}
    assert c["flat"] == (174, 0.0, -24)
    assert c["ones"] == F.LLR_ONES_ROWS and c["alias"]
    assert F.llr_grid().min() == -240.0
    # ties among the eight tones of a quantised payload give LLRs of exactly zero
    llr = O.db_to_llr(O.payload(F.quantised_grid(), 400, 0))[0]
    assert (llr == 0).sum() >= 5 and not np.isnan(llr).any()
    trip = F.llr_triples(4, 300)
    assert len(trip) == 300 and len({t[0] for t in trip[:65]}) == 4 and [t[0] for t in trip] != sorted(t[0] for t in trip)


def test_zero_spectrum_resolves_every_tie_to_the_first_trial():
    assert F.fine_zero_census(W.oracle_config()) == {(0, -8, -32, 3)}


def test_single_bin_spectra_give_other_tweaks():
    ocfg = W.oracle_config()
    s = F.spectra()
    assert s.shape == (len(F.SPECTRA), O.SPEC_BINS)
    got = {(name, f0, h0): O.fine(s[i], f0, h0, ocfg) for i, name in enumerate(F.SPECTRA) for f0 in F.FINE_F0 for h0 in (0, -141)}
    tweaks = {(r["ttweak"], r["ftweak"]) for r in got.values()}
    assert len(tweaks) >= 4, tweaks
