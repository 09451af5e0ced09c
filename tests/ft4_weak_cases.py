"""Fixtures of the FT4 weak-search tests (tests/test_ft4_weak.py on the CPU, tests/test_gpu_ft4_weak.py on the GPU): the stage's frames,
the twin's results on them (computed once per process and shared), the error bound that follows from the FFT's amplitude bound, and the
margins of the twin's decisions.  Everything comes from pyft8_amd/ft4.py (the float64 twin) and seeds; nothing is read from disk."""
import functools

import numpy as np

import ft4_cases as cases
from pyft8_amd import ft4

# The parent's asserted bound of the 576-point fp32 LDS FFT (tests/test_gpu_ft4.py AMP_BOUND): a bin's amplitude is off by at most
# 6e-7 of the row's norm sqrt(sum_k |X_k|^2).  For a 576-point transform of 576 samples that norm is 24 ||x||_2 (Parseval).
AMP_BOUND = 6e-7
# the stage's threshold: low enough that noise peaks are candidates too (10, 12 and 16 on the signal, noise and edge frames), and chosen on
# the twin alone so that every decision behind the lists is far from a tie (tests/test_ft4_weak.py asserts it)
STAGE_WEAK_MIN = 15.25
F0_RANGE = cases.F0_RANGE
H0_RANGE = cases.H0_RANGE
H0_WIDE = (H0_RANGE[0], 230)           # reaches the signal that starts at +2.6 s and runs past the frame (row 217)
FRAMES = ("six signals", "noise", "all zero", "edges")


@functools.lru_cache(maxsize=None)
def frame(name):
    """six signals: ft4_cases.six(); edges: ft4_cases.demod_frames()'s frame 0 -- a signal from -0.3 s, one from +2.6 s (it runs past sample
    89 999), one at the lowest and one at the highest f0 of the range"""
    return {"six signals": lambda: cases.six()[0], "noise": cases.noise_frame, "all zero": cases.zero_frame,
            "edges": lambda: cases.demod_frames()[0][0]}[name]()


def h0_range(name):
    return H0_WIDE if name == "edges" else H0_RANGE


@functools.lru_cache(maxsize=None)
def twin(name, f0_lo=F0_RANGE[0], f0_hi=F0_RANGE[1], h0_lo=None, h0_hi=None):
    """-> dict(best [nf0], bh [nf0], bound [nf0], gap [nf0]) of a stage frame over the given range (h0: the frame's own by default).
    bound: what |best - the kernel's best| may be (score_bound, the maximum over the bin's block); gap: best minus the highest score of
    the block at another h -- the distance of the bin's h0 decision from a tie."""
    a, b = h0_range(name) if h0_lo is None else (h0_lo, h0_hi)
    x = frame(name)
    fq_lo = max(4 * f0_lo - 2, 0)
    S, sums, nrm = ft4.weak_score_map(x, fq_lo, 4 * (f0_hi - 1) + 2, a, b, full=True)
    B = score_bound(x, S, nrm, a, b)
    best, bh = ft4.weak_best(S, fq_lo, f0_lo, f0_hi, a)
    bound, gap = np.zeros(len(best)), np.zeros(len(best))
    for i, f0 in enumerate(range(f0_lo, f0_hi)):
        lo, hi = max(4 * f0 - 2, 0) - fq_lo, 4 * f0 + 2 - fq_lo
        bound[i] = B[lo:hi].max()
        other = np.delete(S[lo:hi], bh[i] - a, axis=1)
        gap[i] = best[i] - other.max() if other.size else np.inf
    return dict(best=best, bh=bh, bound=bound, gap=gap)


def score_bound(x, score, nrm, h0_lo, h0_hi):
    """|score - the kernel's score| per (fq, h) that follows from the FFT's amplitude bound.  Every grid value of row r is off by at most
    d_r = AMP_BOUND x 24 ||x_r||_2 (x_r: the row's 576 samples, zeros outside the frame).  With S = the sum of the four |B_b| and
    nrm = sqrt(sum of the 64 |W|^2), score = 8 S / nrm:  |dS| <= D1 = the sum of d_r over the 16 sync symbols' rows (a block sum adds four
    values, a magnitude is 1-Lipschitz), |d nrm| <= D2 = sqrt(4 sum d_r^2) (the norm of the 64 errors), hence
    |d score| <= (8 D1 + score D2) / (nrm - D2), infinite where nrm <= D2; 0 on digital silence (nrm = D2 = 0: the score is exactly 0)."""
    x = np.asarray(x, np.float64)
    hs = np.arange(h0_lo, h0_hi)
    rows = np.arange(h0_lo + 4, h0_hi + 4 * (ft4.NSYM - 2))
    d = AMP_BOUND * 24.0 * np.sqrt((ft4._symbols(x, ft4.HOP * rows) ** 2).sum(axis=1))
    D1, D2 = np.zeros(len(hs)), np.zeros(len(hs))
    for sym, _ in ft4.SYNC_SYMS:
        dr = d[hs + 4 * sym - rows[0]]
        D1 += dr
        D2 += 4.0 * dr * dr
    D2 = np.sqrt(D2)
    den = nrm - D2[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(den > 0, (8.0 * D1[None, :] + score * D2[None, :]) / np.where(den > 0, den, 1.0), np.inf)
    return np.where((nrm == 0) & (D2[None, :] == 0), 0.0, out)


def best_bound(t):
    """the bound of a comparison with the kernel's float32 best: the score's own bound plus the rounding of the stored value"""
    return t["bound"] + np.abs(t["best"]) * 2.0 ** -23


def list_margin(t, weak_min, max_cands):
    """The smallest (twin score difference) / (sum of the two scores' bounds) over the decisions behind the candidate list: the
    threshold at every bin, the neighbour suppression of every bin at or above it, the order of the kept and the cut at max_cands.
    A value above 1 says that no decision lies closer to a tie than the two bounds together."""
    best, bb = t["best"], best_bound(t)
    n, worst = len(best), np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        thr = np.abs(best - weak_min) / bb
    worst = min(worst, float(np.nanmin(np.where(bb > 0, thr, np.inf))))
    above = [i for i in range(n) if best[i] >= weak_min]
    kept = [i for i in above if not (i > 0 and best[i - 1] >= best[i]) and not (i + 1 < n and best[i + 1] > best[i])]
    for i in above:
        for j in (i - 1, i + 1):
            if 0 <= j < n:
                worst = min(worst, abs(best[i] - best[j]) / (bb[i] + bb[j]))
    order = sorted(kept, key=lambda i: -best[i])
    for a, b in zip(order, order[1:max_cands + 1]):
        worst = min(worst, (best[a] - best[b]) / (bb[a] + bb[b]))
    return worst


def h0_clear(t):
    """per bin: the twin's h0 decision is further from a tie than twice the bound"""
    return t["gap"] > 2.0 * best_bound(t)


def twin_list(t, f0_lo, weak_min, max_cands):
    return ft4._keep(t["best"], t["bh"], f0_lo, weak_min, max_cands)


@functools.lru_cache(maxsize=None)
def strongest():
    """(f0, h0, score) of the six-signal frame's best candidate"""
    return twin_list(twin("six signals"), F0_RANGE[0], STAGE_WEAK_MIN, 256)[0]


def narrow_ranges():
    """(f0_lo, f0_hi, h0_lo, h0_hi): the one-bin range at the strongest signal, and the whole band with the h0 range narrowed to its row"""
    f0, h0, _ = strongest()
    return [(f0, f0 + 1, H0_RANGE[0], H0_RANGE[1]), (F0_RANGE[0], F0_RANGE[1], h0, h0 + 1)]
