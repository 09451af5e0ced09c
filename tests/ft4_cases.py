"""Fixtures of the FT4 tests (tests/test_ft4.py on the CPU, tests/test_gpu_ft4.py on the GPU): seeded frames, the twin's results on them
(computed once per process and shared), crafted demodulator candidates, raw LLR vectors, and the error bounds that follow from the
grid's bound.  Everything comes from pyft8_amd/ft4.py (the float64 twin) and seeds; nothing is read from disk."""
import functools

import numpy as np

from pyft8_amd import ft4, synth

SIX = (12, 17, 18)                    # make_frame indices of the 6-signal frames (-8 .. +5 dB, >= 150 Hz apart, starts 0.1 .. 1.5 s)
NOISE = 1000                          # make_frame index of the noise-only frame
# the search tests run above the noise: every per-bin maximum of the fixtures' noise lies far below, every planted signal far above
SEARCH_SYNC_MIN = 160.0
F0_RANGE = ft4.freq_range_to_f0()     # (2, 567)
H0_RANGE = ft4.time_range_to_h0()     # (-42, 168)

# one word of every opt-in message type (synth.pack77_ext), with its msg_types bit name
EXT_TEXTS = [("free_text", "TNX BOB 73 GL"), ("dxpedition", "K1ABC RR73; W9XYZ <KH1/KH7Z> -08"), ("field_day", "K1ABC W9XYZ R 17B EMA"),
             ("telemetry", "123456789ABCDEF012"), ("rtty_ru", "TU; K1ABC W9XYZ 579 WI"), ("eu_vhf", "<PA3XYZ> <G4ABC> R 590003 IO91NP")]


def ext_words():
    return [(name, text, synth.pack77_ext(text, "telemetry" if name == "telemetry" else None)) for name, text in EXT_TEXTS]


@functools.lru_cache(maxsize=None)
def six(index=SIX[0]):
    """-> (audio int16 [90000], truth) of a 6-signal frame"""
    return ft4.make_frame(index, n_signals=6, snr_range=(-8.0, 5.0), return_truth=True)


@functools.lru_cache(maxsize=None)
def noise_frame():
    return ft4.make_frame(NOISE, n_signals=0)


def zero_frame():
    return np.zeros(ft4.NFRAME, np.int16)


@functools.lru_cache(maxsize=None)
def clipped_frame():
    """full scale: a strong carrier plus noise, most samples at the rails"""
    rng = np.random.Generator(np.random.Philox(key=ft4.SEED_BASE + 555))
    n = np.arange(ft4.NFRAME)
    x = 90000.0 * np.sin(2 * np.pi * 1234.5 * n / ft4.FS) + 20000.0 * rng.standard_normal(ft4.NFRAME)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def grid_frames():
    """the B = 3 batch of the grid test -> (audio [3, 90000], P64 [3, 618, 577])"""
    a = np.stack([six()[0], zero_frame(), clipped_frame()])
    return a, np.stack([ft4.grid_power(x) for x in a])


@functools.lru_cache(maxsize=None)
def six_grid(index=SIX[0]):
    """-> (P64, dB64) of a 6-signal frame"""
    P = ft4.grid_power(six(index)[0])
    return P, ft4.grid_db(P)


@functools.lru_cache(maxsize=None)
def twin_search(index, f0_lo, f0_hi, h0_lo, h0_hi, sync_min, max_cands):
    """the twin's search on a 6-signal frame -> (candidates [(f0, h0, score)], best [nf0], best h0 [nf0], score map)"""
    return ft4.search(six_grid(index)[1], f0_lo, f0_hi, h0_lo, h0_hi, sync_min, max_cands, full=True)


def grid_errors(P, P64):
    """The two error measures of a grid against the twin's, per row (rows whose P64 is all zero: exact zeros wanted, reported as 0 / inf):
    power  max_k |P - P64| / max_k P64 -- the measure of the grid test, dominated by the row's strongest bin;
    amp    max_k | sqrt(P) - sqrt(P64) | / sqrt(sum_k P64) -- the amplitude error of a bin against the row's norm, which is what a
           float32 FFT's rounding is proportional to; it bounds the dB error of WEAK bins too (db_error_map), which the power measure
           does not: a noise bin 60 dB below a carrier may be off by the carrier's whole error there."""
    P = np.asarray(P, np.float64)
    top, tot = P64.max(axis=1), P64.sum(axis=1)
    zero = tot == 0
    bad = np.where((np.abs(P) > 0).any(axis=1), np.inf, 0.0)
    power = np.where(zero, bad, np.abs(P - P64).max(axis=1) / np.where(zero, 1.0, top))
    amp = np.where(zero, bad, np.abs(np.sqrt(P) - np.sqrt(P64)).max(axis=1) / np.sqrt(np.where(zero, 1.0, tot)))
    return power, amp


def db_error_map(P64, amp_bound):
    """What the grid's amplitude bound (| sqrt(P) - sqrt(P64) | <= amp_bound x sqrt(the row's sum of P64)) allows each dB value to be off
    by: with x = amp_bound sqrt(sum) / sqrt(P64), |dB - dB64| <= -20 log10(1 - x), infinite from x = 1 on."""
    x = amp_bound * np.sqrt(P64.sum(axis=1, keepdims=True)) / np.sqrt(np.maximum(P64, 1e-300))
    return np.where(x < 1.0, -20.0 * np.log10(np.maximum(1.0 - x, 1e-300)), np.inf)


def score_bound_map(P64, amp_bound, f0_lo, f0_hi, h0_lo, h0_hi):
    """The bound of |score - twin score| per (f0, h0) that follows from the grid's amplitude bound on the 16 dB terms: each term is its
    own tone's dB error plus a third of the other three tones'."""
    return ft4.score_map(db_error_map(P64, amp_bound), f0_lo, f0_hi, h0_lo, h0_hi, weights=(1.0, 1.0 / 3.0))


def search_margin(cands, best, bh, bound, f0_lo, h0_lo, sync_min, max_cands):
    """The smallest (twin score difference) / (sum of the two scores' bounds) over the decisions of a search result: the order of the
    kept candidates, the cut at max_cands, the threshold and the neighbour suppression of every bin at or above it."""
    b_at = lambda i: bound[i, bh[i] - h0_lo]                       # the bound of bin i's best score
    worst = np.inf
    above = [i for i in range(len(best)) if best[i] >= sync_min]
    kept = [i for i in above if not (i > 0 and best[i - 1] >= best[i]) and not (i + 1 < len(best) and best[i + 1] > best[i])]
    order = sorted(kept, key=lambda i: -best[i])
    assert [(f0_lo + i) for i in order[:max_cands]] == [c[0] for c in cands]
    for a, b in zip(order, order[1:max_cands + 1]):                # order, and the cut (the first one left out)
        worst = min(worst, (best[a] - best[b]) / (b_at(a) + b_at(b)))
    for i in range(len(best)):                                     # threshold
        worst = min(worst, abs(best[i] - sync_min) / b_at(i))
    for i in above:                                                # neighbour suppression, either outcome
        for j in (i - 1, i + 1):
            if 0 <= j < len(best):
                worst = min(worst, abs(best[i] - best[j]) / (b_at(i) + b_at(j)))
    return worst


# ----------------------------------------------------------------------------- crafted demodulator candidates
DEMOD_WORD = synth.pack77("CQ", "K1ABC", "FN42")


@functools.lru_cache(maxsize=None)
def demod_frames():
    """-> (audio [3, 90000], candidates [(frame, f0, h0, what)]): frame 0 holds four signals at 0 dB -- one that starts at -0.3 s (the ramp
    and part of block a lie before the frame), one that starts at +2.6 s (it runs past sample 89 999), one at the lowest and one at the
    highest f0 of the range -- frame 1 is noise, frame 2 all zero."""
    lo, hi = F0_RANGE[0], F0_RANGE[1] - 1
    sigs = [(DEMOD_WORD, 1000.0, -0.3, 0.0), (DEMOD_WORD, 1500.0, 2.6, 0.0), (DEMOD_WORD, lo * ft4.BIN_HZ + 1.0, 0.7, 0.0),
            (DEMOD_WORD, hi * ft4.BIN_HZ - 1.0, 1.1, 0.0)]
    a = np.stack([ft4.frame_with_signals(7, sigs), noise_frame(), zero_frame()])
    row = lambda t: int(np.rint(t * ft4.FS / ft4.HOP))
    cands = [(0, 96, row(-0.3), "starts before the frame"), (0, 144, row(2.6), "runs past the frame"), (0, lo, row(0.7), "lowest f0"),
             (0, hi, row(1.1), "highest f0"), (1, 300, 40, "noise"), (2, 200, 30, "all-zero frame")]
    return a, cands


def demod_candidates(n):
    """n triples: the six crafted ones, then the same signals at neighbouring rows and bins (other trials win there)"""
    a, base = demod_frames()
    out = [c[:3] for c in base]
    k = 0
    while len(out) < n:
        f, f0, h0, _ = base[k % 4]
        step = 1 + k // 4
        out.append((f, min(max(f0 + (step % 3) - 1, F0_RANGE[0]), F0_RANGE[1] - 1), h0 + (step % 5) - 2))
        k += 1
    return a, out[:n]


@functools.lru_cache(maxsize=None)
def twin_demod(frame, f0, h0):
    return ft4.demod(demod_frames()[0][frame], f0, h0)


# ----------------------------------------------------------------------------- raw LLR vectors of the back end
def codeword_bits(word77, scrambled=True):
    cw = synth.encode174(int(word77) ^ (ft4.RVEC if scrambled else 0))
    return np.array([(cw >> (173 - i)) & 1 for i in range(174)], np.float64)


def noisy_llrs(words, sigma, seed, scrambled=True):
    """BPSK LLRs of the words' codewords (positive = bit 1) in Gaussian noise of standard deviation sigma, scaled as the receivers
    scale theirs (2.83 / std) -> float32 [n, 174]"""
    rng = np.random.Generator(np.random.Philox(key=0x4C4C5200 + seed))
    out = []
    for w in words:
        v = (2.0 * codeword_bits(w, scrambled) - 1.0) + sigma * rng.standard_normal(174)
        out.append(ft4.LLR_SCALE * v / np.std(v))
    return np.array(out, np.float32)


def random_words(n, seed):
    rng = np.random.Generator(np.random.Philox(key=0x574F5244 + seed))
    return [synth.pack77(*synth.random_message(rng)) for _ in range(n)]


def split_words(words):
    return (np.array([w & (2 ** 64 - 1) for w in words], np.uint64), np.array([w >> 64 for w in words], np.uint64))


def join_words(lo, hi):
    return [(int(h) << 64) | int(l) for l, h in zip(lo, hi)]
