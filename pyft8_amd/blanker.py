"""Noise blanker (ft8rx_blank, csrc/kernels/blanker.hpp): the numpy twin of the kernels, the normalisation of
Receiver(noise_blanker=), and the impulse-noise recipe the measurements and tests use.  No GPU needed.

A frame is 180000 int16 samples = 375 blocks of 480; frames are independent.  Everything is integer arithmetic (int64 here, int32 on
the device), so twin and kernels agree bit for bit:
    m_b   = the element at sorted position 240 of |x| over block b          (|-32768| = 32768)
    L_b   = the element at sorted position 2 of m[clamp(b + d, 0, 374)], d = -2 .. 2
    hit   = L_b > 0 and 256 |x[n]| > threshold_q8 L_b
    w[n]  = 0 for d[n] <= guard, T[d[n] - guard] for guard < d[n] <= guard + taper, 32768 beyond (d = distance to the nearest hit)
    y[n]  = (x[n] w[n] + 16384) >> 15
"""
import numpy as np

from . import _lib

NSAMP, BLOCK, N_BLOCKS = _lib.NSAMP, 480, 375
THRESHOLD_DEFAULT, GUARD_DEFAULT, TAPER_DEFAULT = 8.0, 6, 6           # include/ft8rx.h FT8RX_BLANK_*_DEFAULT
MIN_THRESHOLD_Q8, MAX_THRESHOLD_Q8, MAX_GUARD, MAX_TAPER = 512, 16384, 64, 64
IMPULSE_SHAPE = (0.5, 1.0, -0.7, 0.3, -0.1)


def check(threshold=THRESHOLD_DEFAULT, guard=GUARD_DEFAULT, taper=TAPER_DEFAULT):
    """(threshold k, guard, taper) -> (threshold_q8, guard, taper) as ft8rx_blank takes them; anything outside the definition is
    refused, naming the argument."""
    try:
        q8 = float(np.rint(256.0 * float(threshold)))
    except (TypeError, ValueError):
        q8 = np.nan
    if not MIN_THRESHOLD_Q8 <= q8 <= MAX_THRESHOLD_Q8:
        raise _lib.Ft8rxError(f"noise blanker: threshold={threshold!r}: k with 256 k in [{MIN_THRESHOLD_Q8}, {MAX_THRESHOLD_Q8}] (2 .. 64)")
    out = [int(q8)]
    for name, v, hi in (("guard", guard, MAX_GUARD), ("taper", taper, MAX_TAPER)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= hi:
            raise _lib.Ft8rxError(f"noise blanker: {name}={v!r}: an integer in [0, {hi}]")
        out.append(int(v))
    return tuple(out)


def params(noise_blanker):
    """The noise_blanker kwarg of Receiver -> None (off) or (threshold_q8, guard, taper): None / False = off, True = the defaults, a
    number = the threshold k, a dict of threshold / guard / taper = those (what it leaves out keeps its default)."""
    if noise_blanker is None or noise_blanker is False:
        return None
    if noise_blanker is True:
        return check()
    if isinstance(noise_blanker, dict):
        bad = set(noise_blanker) - {"threshold", "guard", "taper"}
        if bad:
            raise _lib.Ft8rxError(f"noise_blanker: unknown key(s) {sorted(bad)}; known are threshold, guard, taper")
        return check(**noise_blanker)
    if isinstance(noise_blanker, (int, float, np.integer, np.floating)):
        return check(threshold=noise_blanker)
    raise _lib.Ft8rxError(f"noise_blanker={noise_blanker!r}: None, True, a threshold k or a dict of threshold, guard, taper")


def taper_table(taper):
    """T[1 .. taper] (int64 [taper]): rint(32768 * 0.5 (1 - cos(pi j / (taper + 1)))), in double, rounded once (= ft8rx_blank_taper)"""
    j = np.arange(1, int(taper) + 1, dtype=np.float64)
    return np.rint(32768.0 * 0.5 * (1.0 - np.cos(np.pi * j / (int(taper) + 1.0)))).astype(np.int64)


def levels_of(x):
    """x int [B, 180000] -> (m, L) int64 [B, 375] each"""
    a = np.abs(np.asarray(x, np.int64)).reshape(len(x), N_BLOCKS, BLOCK)
    m = np.sort(a, axis=2)[:, :, BLOCK // 2]
    idx = np.clip(np.arange(N_BLOCKS)[:, None] + np.arange(-2, 3)[None, :], 0, N_BLOCKS - 1)
    return m, np.sort(m[:, idx], axis=2)[:, :, 2]


def weights(hit, guard, taper):
    """hit bool [B, 180000] -> w int64 [B, 180000]: the gate of each frame's own hits"""
    B, N = hit.shape
    n = np.arange(N, dtype=np.int64)[None, :]
    far = np.int64(1) << 40
    last = np.maximum.accumulate(np.where(hit, n, -far), axis=1)                           # the nearest hit at or before n
    nxt = np.minimum.accumulate(np.where(hit, n, far)[:, ::-1], axis=1)[:, ::-1]           # ... at or after n
    d = np.minimum(n - last, nxt - n)
    tab = np.concatenate([np.zeros(guard + 1, np.int64), taper_table(taper), [32768]])
    return tab[np.minimum(d, guard + taper + 1)]


def reference(x, threshold=THRESHOLD_DEFAULT, guard=GUARD_DEFAULT, taper=TAPER_DEFAULT):
    """The blanker on frames x (int16 [B, 180000], or one frame [180000]) -> (y int16 like x, stats int64 [B, 4], levels int64
    [B, 375, 2] = (m_b, L_b)); stats = hits, samples with w < 32768, samples with w = 0, blocks with L_b = 0."""
    q8, guard, taper = check(threshold, guard, taper)
    x = np.asarray(x)
    one = x.ndim == 1
    xs = np.asarray(x[None] if one else x, np.int64)
    if xs.ndim != 2 or xs.shape[1] != NSAMP or np.abs(xs).max(initial=0) > 32768 or xs.max(initial=0) > 32767:
        raise _lib.Ft8rxError(f"blanker.reference: frames must be int16 [n_frames, {NSAMP}], got shape {x.shape}")
    m, L = levels_of(xs)
    Ls = np.repeat(L, BLOCK, axis=1)
    hit = (Ls > 0) & (256 * np.abs(xs) > q8 * Ls)
    w = weights(hit, guard, taper)
    y = ((xs * w + 16384) >> 15).astype(np.int16)
    stats = np.stack([hit.sum(axis=1), (w < 32768).sum(axis=1), (w == 0).sum(axis=1), (L == 0).sum(axis=1)], axis=1).astype(np.int64)
    return (y[0] if one else y), stats, np.stack([m, L], axis=2)


def add_impulses(frame, rng, rate=100.0, peak_sigma=30.0):
    """Impulse noise on one frame (int16 [180000]) -> int16 [180000]: a Poisson process of `rate` impulses per second, each of the
    shape IMPULSE_SHAPE with the peak peak_sigma sigma U[0.5, 1.5] and a random sign, sigma = median |x| / 0.6745 (the noise level of
    the frame); the sum is rounded and clipped to int16.  rng: a numpy Generator."""
    x = np.asarray(frame, np.int16)
    sigma = float(np.median(np.abs(x.astype(np.int64)))) / 0.6745
    n = int(rng.poisson(rate * len(x) / 12000.0))
    pos = rng.integers(0, len(x), n)
    amp = peak_sigma * sigma * rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
    y = x.astype(np.float64)
    for k, s in enumerate(IMPULSE_SHAPE):
        ok = pos + k < len(x)
        np.add.at(y, pos[ok] + k, s * amp[ok])
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16)
