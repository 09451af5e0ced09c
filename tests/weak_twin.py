"""Numpy twin of weak mode (ft8rx_set_weak): the three-block sync score (k_sync3) and the joint fine scan
(k_fine_weak), composed from the oracle's own entries -- its dB grid (spectrogram), cycle spectrum, the reference-defined 79 x 8 grid of
any (fb, tb) (ft8o_fine_grid) and _dB_to_llr (db_to_llr) -- with the new scores and picks written out here in numpy."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle as O
from pyft8_amd import _lib

COSTAS = (3, 1, 4, 0, 6, 5, 2)
W6 = float(np.float32(-1.0 / 6.0))                 # np.float32(-1/6) as a double (kernels/common.hpp: W6)
PAYSYM = np.array(list(range(7, 36)) + list(range(43, 72)))
FTS = tuple(range(-56, 57, 8))                      # frequency tweaks (outer), 1/16 Hz
TTS = tuple(range(-16, 17, 2))                      # time tweaks (inner), 5 ms


def _rows(grid, rows):
    """grid rows with grid_at's rules: wrap modulo 750, rows outside 1 .. 375 read 1.0 (columns beyond the grid: 0, by padding)."""
    r = np.mod(rows, 750)
    inside = (r >= 1) & (r <= 375)
    g = np.concatenate([grid, np.zeros((grid.shape[0], 32), np.float32)], axis=1).astype(np.float64)
    out = g[np.where(inside, r, 1)]
    out[~inside, :grid.shape[1]] = 1.0
    return out


def sync3_scores(grid, f0_lo, f0_hi, h0_lo, h0_hi):
    """-> (score float32 [f0_hi - f0_lo], h0 int32): per f0 the first strict maximum over h0 (from 0) of the three-block score."""
    grid = np.asarray(grid, np.float32)
    f0 = np.arange(f0_lo, f0_hi)
    h0 = np.arange(h0_lo, h0_hi)
    s1 = np.zeros((len(h0), len(f0)))
    ts = np.zeros((len(h0), len(f0)))
    for b in range(3):                              # fp64, in the order b, s, k
        for s in range(7):
            R = _rows(grid, h0 + 4 + 144 * b + 4 * s)
            t = np.zeros((len(h0), len(f0)))
            for k in range(14):
                t = t + R[:, f0 + k]
            ts = ts + t
            c = COSTAS[s]
            s1 = s1 + (R[:, f0 + 2 * c] + R[:, f0 + 2 * c + 1])
    score = (s1 + W6 * (ts - s1)).astype(np.float32)
    best = np.zeros(len(f0), np.float32)
    bh = np.zeros(len(f0), np.int32)
    for i in range(len(h0)):
        m = score[i] > best
        best = np.where(m, score[i], best)
        bh = np.where(m, h0[i], bh)
    return best, bh


def search(grid, cfg, sync_min):
    """k_sync3 + k_topk: [(f0, h0, score)] above sync_min, stably sorted by score descending, cut at max_cands."""
    sc, h0 = sync3_scores(grid, cfg.f0_lo, cfg.f0_hi, cfg.h0_lo, cfg.h0_hi)
    keep = [(cfg.f0_lo + i, int(h0[i]), float(sc[i])) for i in range(len(sc)) if sc[i] > np.float32(sync_min)]
    keep.sort(key=lambda c: -c[2])
    return keep[:cfg.max_cands]


def fine_grid(spec, fb, tb, ocfg):
    """ft8o_fine_grid: the 79 x 8 grid the reference forms for spectrum origin fb and time origin tb."""
    g = np.zeros((79, 8), np.float32)
    sc = C.c_float()
    O.lib(O._wide(spec=spec)).ft8o_fine_grid(O._p(spec.view(np.float32)), C.byref(ocfg), int(fb), int(tb), O._p(g), C.byref(sc))
    return g


def score3(g):
    """fine_score's per-symbol (on, off) arithmetic over the 21 Costas symbols: b ascending, then a, fp64, one rounding."""
    s1 = s2 = 0.0
    for b in range(3):
        for a in range(7):
            row, c = g[36 * b + a], COSTAS[a]
            off = 0.0
            for q in range(7):
                if q != c:
                    off += float(row[q])
            s1 += float(row[c])
            s2 += off
    return np.float32(s1 + W6 * s2)


def fine_weak(spec, f0, h0, ocfg):
    """k_fine_weak for one candidate -> dict as Handle.fine(weak=True) returns per triple (ret 1 / 0: no sd gate)."""
    spec = np.ascontiguousarray(spec, np.complex64)
    fb0, tb0 = 50 * int(f0), 8 * int(h0) + (1 if h0 < 0 else 0)
    best, bft, btt = None, 0, 0
    for ft in FTS:
        if fb0 + ft < 150:                          # the slice would start below bin 0: not scanned
            continue
        for tt in TTS:
            v = score3(fine_grid(spec, fb0 + ft, tb0 + tt, ocfg))
            if best is None or v > best:
                best, bft, btt = v, ft, tt
    g = fine_grid(spec, fb0 + bft, tb0 + btt, ocfg)
    nsync = sum(int(np.argmax(g[36 * b + a]) == COSTAS[a]) for b in range(3) for a in range(7))
    out = dict(ret=0, ttweak=btt, ftweak=bft, nsync=nsync, llr=np.zeros(174, np.float32), sd=0.0, snr=0, sgrid=g, score=best)
    if nsync > 6:
        p = np.float32(20.0) * O.log10f(g[PAYSYM]).reshape(-1)
        llr, sd, snr, _ = O.db_to_llr(p)
        out.update(ret=1, llr=llr, sd=np.float32(sd), snr=snr)
    return out


def oracle_config(wide=False):
    c = O.default_config(**_lib.fft_plans())
    if wide:
        c.f0_hi = _lib.MAX_F0_WIDE
    return c


def fine_weak_many(specs, trip, ocfg, workers=16):
    """fine_weak over (frame, f0, h0) triples; the oracle's C entries release the GIL, so threads run them side by side."""
    fine_weak(specs[trip[0][0]], trip[0][1], trip[0][2], ocfg)          # first call initialises the oracle's static tables
    with ThreadPoolExecutor(workers) as ex:
        return list(ex.map(lambda t: fine_weak(specs[t[0]], t[1], t[2], ocfg), trip))
