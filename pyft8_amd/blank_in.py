"""Input-rate noise blanker (ft8rx_blank_in*, csrc/kernels/blank_in.hpp): the numpy twin of the kernels, the
release rule of the stream, the normalisation of Receiver(input_blanker=), and the impulse recipe for wide-rate samples.  No GPU needed.

One stream of raw integer samples at its own rate: real int16 [n], or (I, Q) pairs [n, 2] of int16, uint8 or int8.  Everything is
integer arithmetic (int64 here, int32 on the device), so twin and kernels agree bit for bit:
    c     = x (int16), s (int8), 2 u - 255 (uint8)
    a[n]  = |c| (real) or |cI| + |cQ| (IQ); 0 for every index outside the stream
    m_b   = the element at sorted position B / 2 of a over block b = [b B, (b + 1) B) of the ABSOLUTE index
    L_b   = the element at sorted position 2 of m[b - 2 .. b + 2] (no clamping: m = 0 outside the stream)
    hit   = L_b > 0 and 256 a[n] > threshold_q8 L_b
    w[n]  = 0 for d[n] <= guard, T[d[n] - guard] for guard < d[n] <= guard + taper, 32768 beyond (d = distance to the nearest hit)
    c'    = (c w[n] + 16384) >> 15 per component; stored as int16 / int8 c', uint8 (c' + 255) >> 1
"""
import numpy as np

from . import _lib, blanker
from . import kinds as _k
from .kinds import REAL_I16, IQ_I16, WIDE_REAL_I16, WIDE_IQ_I16, WIDE_IQ_U8, WIDE_IQ_I8, components, store  # noqa: F401 -- the integer kinds

KINDS, KIND_NAMES, _DTYPE = _k.view((REAL_I16, IQ_I16, WIDE_REAL_I16, WIDE_IQ_I16, WIDE_IQ_U8, WIDE_IQ_I8))
BLOCK_DEFAULT, MIN_BLOCK, MAX_BLOCK = 1024, 256, 4096             # FT8RX_BLANK_IN_*
THRESHOLD_DEFAULT_REAL, THRESHOLD_DEFAULT_IQ = _k.BLANK_IN_THRESHOLD_REAL, _k.BLANK_IN_THRESHOLD_IQ
GUARD_DEFAULT, TAPER_DEFAULT = 6, 6
MEDIAN_REAL, MEDIAN_IQ = 0.6745, 1.4866                           # the median of |x| and of |I| + |Q| in sigma (Gaussian noise)


def _kind(kind):
    if kind not in KINDS:
        raise _lib.Ft8rxError(f"input blanker: kind={kind!r} is not an integer kind (real int16, IQ int16, IQ uint8, IQ int8)")
    return kind


def is_iq(kind):
    return _k.is_iq(_kind(kind))


def threshold_default(kind):
    return _k.blank_in_threshold(_kind(kind))


def false_hit_probability(k, iq):
    """P(hit) of one sample of Gaussian noise at threshold k: real erfc(k 0.6745 / sqrt 2); IQ 1 - (1 - erfc(k 1.4866 / 2))^2, the
    bound by max(|I|, |Q|) >= (|I| + |Q|) / 2."""
    from math import erfc, sqrt
    if not iq:
        return erfc(k * MEDIAN_REAL / sqrt(2.0))
    p = erfc(k * MEDIAN_IQ / 2.0)
    return 1.0 - (1.0 - p) ** 2


def block_for_rate(sample_rate):
    """the smallest power of two >= sample_rate / 1000, clamped to 256 .. 4096"""
    b = MIN_BLOCK
    while b < MAX_BLOCK and b * 1000 < sample_rate:
        b *= 2
    return b


def check(kind, block=BLOCK_DEFAULT, threshold=None, guard=GUARD_DEFAULT, taper=TAPER_DEFAULT):
    """-> (block, threshold_q8, guard, taper) as ft8rx_blank_in takes them; anything outside the definition is refused, naming the
    argument.  threshold None = the kind's default (k = 8 real, 5.5 IQ)."""
    _kind(kind)
    if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or not MIN_BLOCK <= int(block) <= MAX_BLOCK or int(block) & (int(block) - 1):
        raise _lib.Ft8rxError(f"input blanker: block={block!r}: a power of two in [{MIN_BLOCK}, {MAX_BLOCK}]")
    k = threshold_default(kind) if threshold is None else threshold
    try:
        q8, g, r = blanker.check(k, guard, taper)
    except _lib.Ft8rxError as e:
        raise _lib.Ft8rxError(str(e).replace("noise blanker:", "input blanker:")) from None
    return int(block), q8, g, r


def params(input_blanker, kind, sample_rate):
    """The input_blanker kwarg -> None (off) or (block, threshold_q8, guard, taper): None / False = off, True = the defaults with
    block = block_for_rate(sample_rate), a number = the threshold k, a dict of threshold / guard / taper / block."""
    if input_blanker is None or input_blanker is False:
        return None
    block = block_for_rate(sample_rate)
    if input_blanker is True:
        return check(kind, block)
    if isinstance(input_blanker, dict):
        bad = set(input_blanker) - {"threshold", "guard", "taper", "block"}
        if bad:
            raise _lib.Ft8rxError(f"input_blanker: unknown key(s) {sorted(bad)}; known are threshold, guard, taper, block")
        return check(kind, **dict({"block": block}, **input_blanker))
    if isinstance(input_blanker, (int, float, np.integer, np.floating)):
        return check(kind, block, threshold=input_blanker)
    raise _lib.Ft8rxError(f"input_blanker={input_blanker!r}: None, True, a threshold k or a dict of threshold, guard, taper, block")


def released(n_origin, n_end, block, guard, taper):
    """Absolute index of the first sample that is NOT final once the inputs [.., n_end) exist (= ft8rx_blank_in_released): sample n is
    final once every block up to (n + guard + taper) // block + 2 is complete."""
    return max(int(n_origin), (int(n_end) // int(block) - 2) * int(block) - (int(guard) + int(taper)))


def pack(samples, kind):
    """One stream's samples as the C-contiguous array ft8rx_blank_in takes -> (array, n): real int16 [n]; IQ (I, Q) pairs [n, 2]."""
    _kind(kind)
    a = np.asarray(samples)
    if a.dtype.kind in "fc":
        raise _lib.Ft8rxError(f"input blanker: samples of dtype {a.dtype}: the blanker takes the integer kinds only (kind)")
    return _k.pack_stream(a, kind, "input blanker: ONE stream, {form}, got shape {shape}",
                          "input blanker: kind {kind} needs integers in the {dtype} range, got dtype {got}")


def magnitude(c):
    return np.abs(c) if c.ndim == 1 else np.abs(c[:, 0]) + np.abs(c[:, 1])


def _grid(a, n_origin, B, n_blocks):
    """a of the samples [n_origin, n_origin + len(a)) on the block grid from block n_origin // B on, zero outside -> [n_blocks B]"""
    g = np.zeros(n_blocks * B, np.int64)
    off = n_origin - n_origin // B * B
    g[off:off + len(a)] = a
    return g


def _levels(g, B, n_have):
    """g on the block grid -> (m, L) of its blocks; blocks from n_have on have no level yet / lie outside the stream: m = 0"""
    m = np.sort(g.reshape(-1, B), axis=1)[:, B // 2]
    m[n_have:] = 0
    mp = np.concatenate([np.zeros(2, np.int64), m, np.zeros(2, np.int64)])
    win = np.stack([mp[d:d + len(m)] for d in range(5)], axis=1)
    return m, np.sort(win, axis=1)[:, 2]


def reference(x, kind, block=BLOCK_DEFAULT, threshold=None, guard=GUARD_DEFAULT, taper=TAPER_DEFAULT, n_origin=0):
    """The blanker on the whole stream x at once (the definition) -> (y like pack(x), stats int64 [4], levels int64 [n_blocks, 2] =
    (m_b, L_b) of the blocks n_origin // B .. ceil(n_end / B) - 1); stats = hits, samples with w < 32768, samples with w = 0, blocks
    [n_origin // B, n_end // B) with L_b = 0."""
    B, q8, G, R = check(kind, block, threshold, guard, taper)
    a, n = pack(x, kind)
    n_origin = int(n_origin)
    c = components(a, kind)
    b_first, n_end = n_origin // B, n_origin + n
    n_blocks = max(-(-n_end // B) - b_first, 0)
    if n_blocks == 0:
        return a.copy(), np.zeros(4, np.int64), np.zeros((0, 2), np.int64)
    g = _grid(magnitude(c), n_origin, B, n_blocks)
    m, L = _levels(g, B, n_blocks)
    Ls = np.repeat(L, B)
    hit = (Ls > 0) & (256 * g > q8 * Ls)
    off = n_origin - b_first * B
    w = blanker.weights(hit[None, :], G, R)[0][off:off + n]
    y = (c * (w if c.ndim == 1 else w[:, None]) + 16384) >> 15
    n_complete = n_end // B - b_first
    stats = np.array([hit.sum(), (w < 32768).sum(), (w == 0).sum(), (L[:n_complete] == 0).sum()], np.int64)
    return store(y, kind), stats, np.stack([m, L], axis=1)


def reference_stream(chunks, kind, block=BLOCK_DEFAULT, threshold=None, guard=GUARD_DEFAULT, taper=TAPER_DEFAULT, n_origin=0, finish=True):
    """The stream pushed chunk by chunk -> (list of (n_first, released samples) per push, stats): after each push only the blocks
    that are complete have a level, only the blocks two behind them have hits, and the samples `released` allows are gated with the
    hits known so far.  finish: one more entry releases the rest.  The concatenation equals reference() of the concatenation."""
    B, q8, G, R = check(kind, block, threshold, guard, taper)
    n_origin = int(n_origin)
    b_first = n_origin // B
    off = n_origin - b_first * B
    have = np.zeros((0, 2) if is_iq(kind) else (0,), np.int64)
    out, rel, stats = [], n_origin, np.zeros(4, np.int64)
    steps = [(ch, False) for ch in chunks] + ([(None, True)] if finish else [])
    for ch, fin in steps:
        if ch is not None:
            have = np.concatenate([have, components(pack(ch, kind)[0], kind)])
        n_end = n_origin + len(have)
        c_done = n_end // B
        n_lv = (-(-n_end // B) if fin else c_done) - b_first                 # blocks with a level
        n_hit = n_lv if fin else max(c_done - 2 - b_first, 0)                # blocks whose hits are known
        new_rel = n_end if fin else released(n_origin, n_end, B, G, R)
        n_blocks = -(-n_end // B) - b_first + 1
        g = _grid(magnitude(have), n_origin, B, n_blocks)
        m, L = _levels(g, B, n_lv)
        Ls = np.repeat(L, B)
        hit = (Ls > 0) & (256 * g > q8 * Ls)
        hit[n_hit * B:] = False
        w = blanker.weights(hit[None, :], G, R)[0][off + rel - n_origin:off + new_rel - n_origin]
        c = have[rel - n_origin:new_rel - n_origin]
        out.append((rel, store((c * (w if c.ndim == 1 else w[:, None]) + 16384) >> 15, kind)))
        stats[1] += (w < 32768).sum()
        stats[2] += (w == 0).sum()
        stats[0], stats[3] = hit.sum(), (L[:max(min(n_hit, c_done - b_first), 0)] == 0).sum()
        rel = new_rel
    return out, stats


def add_impulses(x, kind, rng, rate_per_s=100.0, sample_rate=240000, peak_sigma=100.0):
    """Impulse noise on wide-rate samples -> samples of the same kind: section 17's Poisson process (`rate_per_s` impulses per second)
    and peak law (peak_sigma sigma U[0.5, 1.5]) on SINGLE input samples, with a random sign (real) or phase (IQ); sigma = the noise
    level per component by the median of a (0.6745 sigma real, 1.4866 sigma IQ); rounded and clipped to the kind's range."""
    a, n = pack(x, kind)
    c = components(a, kind).astype(np.float64)
    iq = is_iq(kind)
    sigma = float(np.median(magnitude(components(a, kind)))) / (MEDIAN_IQ if iq else MEDIAN_REAL)
    k = int(rng.poisson(rate_per_s * n / float(sample_rate)))
    pos = rng.integers(0, max(n, 1), k)
    amp = peak_sigma * sigma * rng.uniform(0.5, 1.5, k)
    if iq:
        ph = rng.uniform(0.0, 2.0 * np.pi, k)
        np.add.at(c, (pos, 0), amp * np.cos(ph))
        np.add.at(c, (pos, 1), amp * np.sin(ph))
    else:
        np.add.at(c, pos, amp * rng.choice([-1.0, 1.0], k))
    if kind == WIDE_IQ_U8:
        return np.clip(np.rint((c + 255.0) / 2.0), 0, 255).astype(np.uint8)
    info = np.iinfo(_DTYPE[kind])
    return np.clip(np.rint(c), info.min, info.max).astype(_DTYPE[kind])
