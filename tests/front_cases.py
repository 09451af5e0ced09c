"""Designed inputs for the front-end kernels (k_sync / k_sync_acc / k_sync3 / k_topk, k_ft4_sync / k_ft4_peaks, k_grid_llr, k_fine /
k_fine_td / k_fine_weak): grids of small integers and spectra of a few bins, on which every sum of a score is exact -- in fp64, after
the cast to fp32, under any operation order -- so that equal scores, attained thresholds and exact zeros are everywhere.  Recorded or
synthesised audio never produces one of them; the kernels' rules for them (first strict maximum, lowest h0 among the thread rows, a
later window only if strictly larger, strict / inclusive thresholds, f0 order among equal scores, the cut inside a run of equal
scores) run with both sides equal only here.

Everything is seeded; nothing is read from disk.  Each builder has a census next to it that counts the cases the fixture holds with
numpy and the oracle alone (tests/test_front_cases.py asserts them on any machine; tests/test_gpu_front_edges.py compares the kernels).

Why the sums are exact.  FT8: cells are integers below 64, s1 and tsum - s1 are integers below 2^20, W6 = (double)float32(-1/6) has 24
significant bits, so W6 (tsum - s1) has at most 44 and s1 + W6 (tsum - s1) is exact in fp64: one rounding, to fp32, whatever the order
of the additions.  FT4: dB cells that are multiples of 3 make (d0 + d1 + d2 + d3) - own = 3 m, and fl(fl(-1/3) 3 m) = -m exactly, so
every score is an integer."""
import ctypes as C
import functools

import numpy as np

import oracle as O

ROWS, COLS, COLS_WIDE = 376, 976, 1920
FT4_ROWS, FT4_COLS = 618, 577
COSTAS = (3, 1, 4, 0, 6, 5, 2)
W6 = float(np.float32(-1.0 / 6.0))
SYNC_WIN = 352                                      # csrc/ft8rx.hip: h0 offsets per k_sync / k_sync_acc launch
FULL_H0 = (-898, 578)                               # FT8RX_MIN_H0 / FT8RX_MAX_H0: five launches
PHILOX_KEY, COARSE_KEY, WIDE_KEY, PERIODIC_KEY = 1, 2, 3, 7


def _philox(key):
    return np.random.Generator(np.random.Philox(key=key))


# ----------------------------------------------------------------------------- FT8 grids
@functools.lru_cache(maxsize=None)
def _draws():
    """One generator, two draws in a fixed order (the FT8 grid's levels, the FT4 grid's levels); the wide FT8 grid's levels come from
    a generator of their own.  The keys are chosen so that the conditions of tests/test_front_cases.py hold."""
    rng = _philox(PHILOX_KEY)
    a = rng.integers(0, 12, size=(ROWS, COLS))
    b = rng.integers(0, 12, size=(FT4_ROWS, FT4_COLS))
    c = _philox(WIDE_KEY).integers(0, 12, size=(ROWS, COLS_WIDE))
    return a, b, c


def quantised_grid(wide=False):
    """376 x 976 (wide: x 1920) float32, cells 3 k with k uniform in 0 .. 11: 155 or so distinct best scores over 928 columns."""
    g = (3 * _draws()[2 if wide else 0]).astype(np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def coarse_grid():
    """376 x 976, two levels {0, 30} (one cell in eight is 30): few distinct scores, many more ties over h0."""
    g = np.where(_philox(COARSE_KEY).integers(0, 8, size=(ROWS, COLS)) == 0, 30.0, 0.0).astype(np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def periodic_grid():
    """376 x 976, row r = base[r % 16] with integer cells 0 .. 9: as long as every row of the correlation lies inside rows 1 .. 375 the
    scores repeat every 16 offsets, so equal maxima meet inside ONE thread row (`score > best` on equal scores), not between rows."""
    base = _philox(PERIODIC_KEY).integers(0, 10, size=(16, COLS)).astype(np.float32)
    g = base[np.arange(ROWS) % 16]
    g.setflags(write=False)
    return g


def flat_grid(value):
    """all 0.0: every score is exactly 0; all 1.0: the grid equals the rows outside it, every score is 14 + W6 84 = -4.2e-7 (W6 is
    float32(-1/6), a little beyond -1/6) -- no candidate either way (the maximum starts at 0.0 and is strict)."""
    g = np.full((ROWS, COLS), value, np.float32)
    g.setflags(write=False)
    return g


def grid_rows(grid, rows):
    """grid rows with the reference's rules (receiver.py:240, 347, 360): wrapped modulo 750, rows outside 1 .. 375 read 1.0; 32 columns
    of zeros are appended (the search tile reads 0 beyond the grid).  -> float64 [len(rows)][cols + 32]"""
    r = np.mod(rows, 750)
    inside = (r >= 1) & (r <= 375)
    g = np.concatenate([grid, np.zeros((grid.shape[0], 32), np.float32)], axis=1).astype(np.float64)
    out = g[np.where(inside, r, 1)]
    out[~inside, :grid.shape[1]] = 1.0
    return out


def score_map(grid, f0_lo, f0_hi, h0_lo, h0_hi):
    """The search score of every (h0, f0) -> float32 [h0_hi - h0_lo][f0_hi - f0_lo]: fp64 sums in the contract's order (s ascending, the
    14-bin window b ascending), rounded once (oracle/ft8_oracle.c: ft8o_sync_search)."""
    f0 = np.arange(f0_lo, f0_hi)
    h0 = np.arange(h0_lo, h0_hi)
    s1 = np.zeros((len(h0), len(f0)))
    ts = np.zeros((len(h0), len(f0)))
    for s in range(7):
        R = grid_rows(grid, h0 + 148 + 4 * s)
        t = np.zeros((len(h0), len(f0)))
        for b in range(14):
            t = t + R[:, f0 + b]
        ts = ts + t
        s1 = s1 + (R[:, f0 + 2 * COSTAS[s]] + R[:, f0 + 2 * COSTAS[s] + 1])
    return (s1 + W6 * (ts - s1)).astype(np.float32)


def best_of_map(S, h0_lo):
    """per column the first strict maximum from 0.0 -> (best float32, h0 int32; (0.0, 0) where no score is positive)"""
    k = np.argmax(S, axis=0)
    best = S[k, np.arange(S.shape[1])]
    pos = best > 0
    return np.where(pos, best, np.float32(0.0)).astype(np.float32), np.where(pos, h0_lo + k, 0).astype(np.int32)


def oracle_columns(grid, cfg_kw, f0_lo, f0_hi):
    """The oracle's per-column result over [f0_lo, f0_hi): ft8o_sync_search with sync_score_min = 0 and max_cands = 2048; a column it
    omits (no positive score) is (0.0, h0 0).  -> (score float32, h0 int32)"""
    kw = dict(cfg_kw)
    kw.update(sync_score_min=0.0, max_cands=2048, f0_lo=f0_lo, f0_hi=f0_hi)
    sc = np.zeros(f0_hi - f0_lo, np.float32)
    h0 = np.zeros(f0_hi - f0_lo, np.int32)
    # (the build is picked by the grid's layout alone: O.sync_search takes f0_hi = 961, the last legal column + 1, for the wide one)
    cfg, out = O.default_config(**kw), (O.Cand * 2048)()
    n = O.lib(grid.shape[-1] == COLS_WIDE).ft8o_sync_search(O._p(np.ascontiguousarray(grid, np.float32)), C.byref(cfg), out)
    for c in out[:n]:
        sc[c.f0_idx - f0_lo], h0[c.f0_idx - f0_lo] = c.score, c.h0_idx
    return sc, h0


def ordered(best, f0_lo, sync_min):
    """k_topk's order: the columns above sync_min (strict), score descending, equal scores in f0 order -> [(f0, score)]"""
    keep = [(f0_lo + i, float(s)) for i, s in enumerate(best) if s > np.float32(sync_min)]
    keep.sort(key=lambda c: -c[1])
    return keep


def search_census(grid, f0_lo, f0_hi, h0_lo, h0_hi, max_cands=(), thresholds=()):
    """Counts of the tie cases a grid holds over a search range (numpy alone):
      columns      columns with a positive best score
      distinct     distinct best scores among them
      h0_tied      columns whose best score is attained at more than one h0
      lower_row    ... of which a later tied h0 of the same launch sits in a lower thread row ((h0 - window start) % 16 smaller than
                   the first's): the merge of the 16 thread rows meets the later one first and must still return the earlier
      same_row     ... of which a later tied h0 sits in the SAME thread row of the same launch (`score > best` on equal scores)
      groups       scores that two or more columns share (k_topk keeps them in f0 order)
      cut          {max_cands: (kept, size) of the run of equal scores the cut falls into, or None if it falls between two runs}
      attained     {threshold: number of columns whose best score equals it}
      alias        columns whose winner has its alias 750 rows later inside the range with the same score: the winner lies in an
                   earlier launch than its alias and must survive it (`bs > best_score[o]`)"""
    S = score_map(grid, f0_lo, f0_hi, h0_lo, h0_hi)
    best, bh = best_of_map(S, h0_lo)
    pos = best > 0
    h0s = np.arange(h0_lo, h0_hi)
    win, row = (h0s - h0_lo) // SYNC_WIN, ((h0s - h0_lo) % SYNC_WIN) % 16
    out = dict(columns=int(pos.sum()), distinct=len(set(best[pos].tolist())), h0_tied=0, lower_row=0, same_row=0, alias=0)
    for i in np.nonzero(pos)[0]:
        tied = np.nonzero(S[:, i] == best[i])[0]
        if len(tied) > 1:
            first, later = tied[0], tied[1:]
            out["h0_tied"] += 1
            out["lower_row"] += int(((row[later] < row[first]) & (win[later] == win[first])).any())
            out["same_row"] += int(((row[later] == row[first]) & (win[later] == win[first])).any())
            out["alias"] += int(((later - first == 750) & (win[later] > win[first])).any())
    vals, counts = np.unique(best[pos], return_counts=True)
    out["groups"] = int((counts > 1).sum())
    order = ordered(best, f0_lo, 0.0)
    out["cut"] = {}
    for m in max_cands:
        if m < len(order) and order[m - 1][1] == order[m][1]:
            run = [k for k, c in enumerate(order) if c[1] == order[m][1]]
            out["cut"][m] = (m - run[0], len(run))
        else:
            out["cut"][m] = None
    out["attained"] = {float(t): int((best == np.float32(t)).sum()) for t in thresholds}
    return out


def attained_threshold(grid, f0_lo, f0_hi, h0_lo, h0_hi):
    """A best score that the most columns share (the highest of those): as sync_score_min it leaves these columns out (the threshold is
    strict), nextafter(t, -inf) takes them."""
    best, _ = best_of_map(score_map(grid, f0_lo, f0_hi, h0_lo, h0_hi), h0_lo)
    vals, counts = np.unique(best[best > 0], return_counts=True)
    return float(vals[counts == counts.max()].max())


# ----------------------------------------------------------------------------- the FT4 dB grid
def ft4_grid():
    """618 x 577 float32, cells 3 k with k uniform in 0 .. 11 (the second draw of the generator)."""
    g = (3 * _draws()[1]).astype(np.float32)
    g.setflags(write=False)
    return g


FT4_SYNC_MIN = 30.0                                 # below every per-bin maximum of ft4_grid(): the neighbour rule alone decides


FT4_NARROW = (100, 137)                             # 37 bins: no multiple of k_ft4_sync's 16-bin tile


def ft4_attained_threshold(db, f0_lo, f0_hi, h0_lo, h0_hi):
    """A score that the most local peaks share (the lowest of those), an integer: FT4's threshold is inclusive, so sync_min = t keeps
    these candidates and t + 1 drops them."""
    from pyft8_amd import ft4
    sc = np.array([c[2] for c in ft4.search(db, f0_lo, f0_hi, h0_lo, h0_hi, 1.0, 2048)])
    vals, counts = np.unique(sc, return_counts=True)
    return float(vals[counts == counts.max()].min())


def ft4_census(db, f0_lo, f0_hi, h0_lo, h0_hi, sync_min, max_cands=2048):
    """Counts on the FT4 twin (pyft8_amd/ft4.py: search):
      kept         candidates kept (threshold, neighbour rule)
      integer      every per-bin best score is an integer
      h0_tied      bins whose best score is attained at more than one h0
      lower_row    ... of which a later tied h0 sits in a lower thread row ((h0 - h0_lo) % 16)
      plateaus     pairs of neighbouring bins with equal best scores, at or above sync_min
      plateau_peaks  ... of which the lower bin is a kept candidate: the pair is a peak, and "a tie goes to the lower bin" decides
      shared       kept candidates that share their score with another kept one
      attained     bins whose best score equals sync_min"""
    from pyft8_amd import ft4
    cands, best, bh, S = ft4.search(db, f0_lo, f0_hi, h0_lo, h0_hi, sync_min, max_cands, full=True)
    tied = lower = 0
    for i in range(len(best)):
        t = np.nonzero(S[i] == best[i])[0]
        if len(t) > 1:
            tied += 1
            lower += int((t[1:] % 16 < t[0] % 16).any())
    sc = np.array([c[2] for c in cands])
    vals, counts = np.unique(sc, return_counts=True)
    return dict(kept=len(cands), integer=bool((best == np.rint(best)).all()), h0_tied=tied, lower_row=lower,
                plateaus=int(((best[1:] == best[:-1]) & (best[1:] >= sync_min)).sum()),
                plateau_peaks=sum(1 for c in cands if c[0] + 1 < f0_hi and best[c[0] + 1 - f0_lo] == c[2]),
                shared=int(counts[counts > 1].sum()), attained=int((best == sync_min).sum()))


# ----------------------------------------------------------------------------- the LLR grid
# (pmax - pmin) of a payload -> the snr the reference reports: (int)(span - 58) truncates toward zero, clamped to +-24
LLR_SPANS = ((33.0, -24), (34.0, -24), (34.5, -23), (57.5, 0), (58.5, 0), (81.9, 23), (82.0, 24), (82.5, 24), (400.0, 24), (240.0, 24))
LLR_F0 = (4, 100, 116, 132, 148, 164, 180, 196, 960, 212)       # one candidate per span, h0 = LLR_H0; payload columns f0 + 1 .. f0 + 15
LLR_H0 = 0
LLR_FLAT = (300, 0)                                                # a candidate whose payload is flat: sd 0, 174 NaNs, snr -24
PAYSYM = tuple(range(7, 36)) + tuple(range(43, 72))


@functools.lru_cache(maxsize=None)
def llr_grid():
    """Flat 0.0 with one payload cell per candidate of LLR_F0 raised to its span (symbol 7 + j, tone j % 8, so the three LLRs it feeds
    differ from candidate to candidate); the last candidate's cell is lowered to -240, the floor of the dB grid, instead."""
    g = np.zeros((ROWS, COLS), np.float32)
    for j, ((span, _), f0) in enumerate(zip(LLR_SPANS, LLR_F0)):
        row, col = LLR_H0 + 4 + 4 * PAYSYM[j], f0 + 1 + 2 * (j % 8)
        g[row, col] = -240.0 if j == len(LLR_SPANS) - 1 else span
    g.setflags(write=False)
    return g


LLR_EDGE_F0 = (4, 960)
LLR_EDGE_H0 = (-37, -32, -31, 86, 87, 100, 713, -787)           # 713 and -787 are aliases of -37 (modulo 750)
LLR_ONES_ROWS = {-37: 2, -32: 1, 100: 4, 713: 2}                  # payload rows read outside rows 1 .. 375: all 1.0


def llr_triples(n_grids, n, seed=5):
    """n (frame, f0, h0) triples in a seeded mixed order: every designed candidate and the flat one on every frame, and the edge
    f0 x h0 product on every frame; n beyond the list's length repeats it."""
    base = [(f0, LLR_H0) for f0 in LLR_F0] + [LLR_FLAT] + [(f0, h0) for f0 in LLR_EDGE_F0 for h0 in LLR_EDGE_H0]
    trip = [(fr, f0, h0) for fr in range(n_grids) for f0, h0 in base]
    order = np.random.default_rng(seed).permutation(len(trip))
    return [trip[order[i % len(trip)]] for i in range(n)]


def llr_census(grid):
    """On the oracle alone: {span: snr} of the designed candidates, the flat candidate's (NaNs, sd, snr), the all-1.0 payload rows per
    edge h0, and whether the alias payloads are identical."""
    spans = {}
    for (span, _), f0 in zip(LLR_SPANS, LLR_F0):
        spans[span] = O.db_to_llr(O.payload(grid, f0, LLR_H0))[2]
    llr, sd, snr, _ = O.db_to_llr(O.payload(grid, *LLR_FLAT))
    ones = {h0: int((O.payload(grid, 400, h0) == 1.0).all(axis=1).sum()) for h0 in LLR_ONES_ROWS}
    alias = all(O.payload(grid, f0, h0).tobytes() == O.payload(grid, f0, -37).tobytes() for f0 in LLR_EDGE_F0 for h0 in (713, -787))
    return dict(spans=spans, flat=(int(np.isnan(llr).sum()), float(sd), int(snr)), ones=ones, alias=alias)


# ----------------------------------------------------------------------------- spectra for the fine sync
FINE_F0 = (4, 400, 958)
FINE_H0 = (0, -140, -141, 220, 221, -898, 577)                    # -140 .. 220: k_fine; beyond: k_fine_td
FINE_AMP = 1.0e6
SPECTRA = ("zero", "tone0", "off2", "ends", "pair", "const")


@functools.lru_cache(maxsize=None)
def spectra():
    """[6][SPEC_BINS] complex64, named by SPECTRA.  A candidate (f0, .) reads the 1064 bins from 50 f0 - 182 on, tone 0 sits at 50 f0; the
    three candidates' slices are disjoint, so each spectrum carries the same design once per f0 of FINE_F0:
      zero    nothing: every metric of every scan is 0 -- all arg-max choices are ties
      tone0   the bin of tone 0, 1e6 + 0j
      off2    the bin two grid columns (100 bins, one tone) above tone 0
      ends    the first and the last bin of the 1064-bin slice: read only at the extreme frequency tweaks
      pair    two equal bins 16 bins below and above tone 0: frequency tweaks of either sign score alike
      const   1024 + 0j in every bin of the spectrum"""
    s = np.zeros((len(SPECTRA), O.SPEC_BINS), np.complex64)
    for f0 in FINE_F0:
        fb0 = 50 * f0
        s[1, fb0] = FINE_AMP
        s[2, fb0 + 100] = FINE_AMP
        s[3, fb0 - 182] = s[3, fb0 - 182 + 1063] = FINE_AMP
        s[4, fb0 - 16] = s[4, fb0 + 16] = FINE_AMP
    s[5, :] = 1024.0
    s.setflags(write=False)
    return s


def fine_triples():
    """(frame, f0, h0): every spectrum x FINE_F0 x FINE_H0"""
    return [(fr, f0, h0) for fr in range(len(SPECTRA)) for f0 in FINE_F0 for h0 in FINE_H0]


def fine_zero_census(ocfg=None):
    """O.fine on the all-zero spectrum for every (f0, h0): the set of (ret, ttweak, ftweak, nsync) results -- one element, the first
    trial of either scan, if every arg-max resolves a tie to its first entry."""
    z = spectra()[0]
    out = set()
    for f0 in FINE_F0:
        for h0 in FINE_H0:
            r = O.fine(z, f0, h0, ocfg)
            out.add((r["ret"], r["ttweak"], r["ftweak"], r["nsync"]))
    return out


# ----------------------------------------------------------------------------- weak mode's three-block score
def score3_map(grid, f0_lo, f0_hi, h0_lo, h0_hi):
    """The three-block score of every (h0, f0) (k_sync3; tests/weak_twin.py: sync3_scores keeps only the maxima) -> float32."""
    f0 = np.arange(f0_lo, f0_hi)
    h0 = np.arange(h0_lo, h0_hi)
    s1 = np.zeros((len(h0), len(f0)))
    ts = np.zeros((len(h0), len(f0)))
    for b in range(3):
        for s in range(7):
            R = grid_rows(grid, h0 + 4 + 144 * b + 4 * s)
            t = np.zeros((len(h0), len(f0)))
            for k in range(14):
                t = t + R[:, f0 + k]
            ts = ts + t
            s1 = s1 + (R[:, f0 + 2 * COSTAS[s]] + R[:, f0 + 2 * COSTAS[s] + 1])
    return (s1 + W6 * (ts - s1)).astype(np.float32)


SYNC3_WIN = 128                                     # kernels/sync_search.hpp: h0 offsets per k_sync3 / k_sync3_acc launch


def weak_census(grid, f0_lo, f0_hi, h0_lo, h0_hi):
    """-> (best, h0, h0_tied, alias): the per-column maxima of the three-block score, the columns whose maximum is attained more than
    once, and those whose winner meets its alias 750 rows later in a later launch."""
    S = score3_map(grid, f0_lo, f0_hi, h0_lo, h0_hi)
    best, bh = best_of_map(S, h0_lo)
    tied = alias = 0
    for i in np.nonzero(best > 0)[0]:
        t = np.nonzero(S[:, i] == best[i])[0]
        tied += int(len(t) > 1)
        alias += int(((t[1:] - t[0] == 750) & (t[1:] // SYNC3_WIN > t[0] // SYNC3_WIN)).any())
    return best, bh, tied, alias
