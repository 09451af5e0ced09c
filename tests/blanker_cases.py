"""Crafted frames for the noise blanker, shared by tests/test_blanker.py (the numpy twin, no GPU) and
tests/test_gpu_blanker.py (ft8rx_blank against the twin, bit for bit).  Every frame is Gaussian noise at sigma = 1000 from a fixed seed
plus planted samples; the positions that depend on guard + taper are planted for the parameter set the frames are built for."""
import numpy as np

from pyft8_amd import blanker

NSAMP, BLOCK = 180000, 480
BIG = 30000                                  # a planted hit: above k = 8 times any noise block's median (~675) by a wide margin
# (k, guard, taper) of the GPU comparison
PARAM_SETS = [(8.0, 6, 6), (2.0, 0, 0), (5.5, 64, 64), (8.0, 0, 64), (8.0, 64, 0)]
# the recipe of the benefit measurement: frames, signals, impulses
RECIPE_FRAMES, RECIPE_SIGNALS, RECIPE_SNR, RECIPE_RATE, RECIPE_PEAK, RECIPE_SEED = (900, 901, 902), 30, (-16, 0), 100.0, 30.0, 17


def noise(seed):
    return np.clip(np.rint(1000.0 * np.random.default_rng(seed).standard_normal(NSAMP)), -32767, 32767).astype(np.int16)


def plant(x, positions, value=BIG):
    for i, n in enumerate(positions):
        x[n] = value if i % 2 == 0 else -value
    return x


def flat_blocks(x, b0, n_blocks, level):
    """blocks b0 .. b0 + n_blocks - 1 become +-level alternating: m_b = level exactly, whatever is planted on a few samples"""
    seg = np.where(np.arange(n_blocks * BLOCK) % 2 == 0, level, -level).astype(np.int16)
    x[b0 * BLOCK:(b0 + n_blocks) * BLOCK] = seg
    return x


def frames(k, guard, taper):
    """name -> int16 [180000] for the parameter set (k, guard, taper)"""
    q8, G, R = blanker.check(k, guard, taper)
    H = G + R
    out = {}
    # hits at the frame's ends and guard + taper inside them
    out["ends"] = plant(noise(1), [0, 1, H, NSAMP - 1 - H, NSAMP - 1])
    # both sides of every block edge
    out["block_edges"] = plant(noise(2), [n for b in range(1, 375) for n in (b * BLOCK - 1, b * BLOCK)])
    # both sides of multiples of 8, 64, 256, 1024, 1920 and 2048 (the sizes a kernel may tile by)
    mult = [8 * 5, 8 * 12345, 64, 64 * 2, 64 * 17, 64 * 1000, 64 * 2811, 64 * 2812, 256, 256 * 5, 256 * 300, 256 * 703, 1024, 1024 * 7, 1024 * 100,
            1024 * 175, 1920, 1920 * 2, 1920 * 50, 1920 * 93, 2048, 2048 * 2, 2048 * 43, 2048 * 87]
    out["tile_edges"] = plant(noise(3), [n for m in mult for n in (m - 1, m)])
    # two hits 1, guard + taper and 2 (guard + taper) + 1 apart (and one more: the gates just do not meet)
    x = noise(4)
    x[[10000, 10001, 30000, 30000 + H, 50000, 50000 + 2 * H + 1, 70000, 70000 + 2 * H + 2]] = [BIG, BIG, BIG, -BIG, -BIG, BIG, BIG, BIG]
    out["pairs"] = x
    # exactly at the threshold (no hit) and one above it (hit): L_b = 1024 over seven flat blocks, 256 |x| = q8 1024 <=> |x| = 4 q8
    x = flat_blocks(noise(5), 100, 7, 1024)
    assert 4 * q8 + 1 <= 32767
    x[103 * BLOCK + 100], x[103 * BLOCK + 300] = 4 * q8, -(4 * q8 + 1)
    x[104 * BLOCK + 100], x[104 * BLOCK + 300] = -4 * q8, 4 * q8 + 1
    out["threshold"] = x
    # -32768, alone and next to another hit
    x = noise(6)
    x[[4000, 8000, 8001]] = [-32768, -32768, 32767]
    out["int16_min"] = x
    # tied medians: 240 x 500 and 240 x 700 (position 240 is the first 700), 241 x 500 and 239 x 700 (it is the last 500), all equal, and
    # 480 x 32768 / 32767
    x = noise(7)
    for b, n_low in ((50, 240), (51, 241), (52, 239)):
        mag = np.where(np.random.default_rng(70 + b).permutation(BLOCK) < n_low, 500, 700)
        x[b * BLOCK:(b + 1) * BLOCK] = mag * np.where(np.arange(BLOCK) % 3 == 0, -1, 1)
    x[200 * BLOCK:201 * BLOCK] = 1234
    x[300 * BLOCK:303 * BLOCK] = np.where(np.arange(3 * BLOCK) % 2 == 0, -32768, 32767)
    out["tied_medians"] = plant(x, [50 * BLOCK + 7, 51 * BLOCK + 7, 52 * BLOCK + 7, 200 * BLOCK + 9])
    out["zeros"] = np.zeros(NSAMP, np.int16)
    # an early pass: zero from sample 153600 + 100 on, hits on both sides of where the smoothed level drops to zero
    x = noise(8)
    x[153600 + 100:] = 0
    out["early_pass"] = plant(x, [153600 - 1, 153600, 153600 + 50, 153600 + 99, 150000, 319 * BLOCK - 1])
    # a 20-ms burst that fills half of one block
    x = noise(9)
    x[250 * BLOCK + 120:250 * BLOCK + 360] = (20000 * np.sign(np.random.default_rng(90).standard_normal(240)) + x[250 * BLOCK + 120:250 * BLOCK + 360] // 4).astype(np.int16)
    out["burst"] = x
    # a quiet start: the first 40 samples cannot hit at any k >= 2 (|x| <= 100 against a median of ~675; few enough to leave m_0 alone)
    x = noise(10)
    x[:40] = np.clip(x[:40], -100, 100)
    out["quiet_start"] = plant(x, [100000])
    return out


ORDER = ["ends", "quiet_start", "tile_edges", "block_edges", "pairs", "threshold", "int16_min", "tied_medians", "zeros", "early_pass", "burst",
         "ends"]

_cache = {}


def batches(k, guard, taper):
    """-> (list of int16 [3, 180000] batches, list of the twin's (y, stats, levels) for each); the first batch has a hit in the last
    sample of frame 0 and none at the start of frame 1.  Computed once per parameter set."""
    key = (k, guard, taper)
    if key not in _cache:
        f = frames(k, guard, taper)
        bs = [np.stack([f[n] for n in ORDER[i:i + 3]]) for i in range(0, len(ORDER), 3)]
        refs = [blanker.reference(b, k, guard, taper) for b in bs]
        for b in bs:
            b.setflags(write=False)
        _cache[key] = (bs, refs)
    return _cache[key]


def recipe():
    """The benefit recipe: -> (clean int16 [3, 180000], noisy int16 [3, 180000], truth = per frame the set of transmitted texts)"""
    if "recipe" not in _cache:
        from pyft8_amd import synth
        rng = np.random.default_rng(RECIPE_SEED)
        clean, noisy, truth = [], [], []
        for i in RECIPE_FRAMES:
            x, t = synth.make_frame(i, n_signals=RECIPE_SIGNALS, snr_range=RECIPE_SNR, return_truth=True)
            clean.append(x)
            noisy.append(blanker.add_impulses(x, rng, RECIPE_RATE, RECIPE_PEAK))
            truth.append({m["msg"] for m in t})
        _cache["recipe"] = (np.stack(clean), np.stack(noisy), truth)
    return _cache["recipe"]
