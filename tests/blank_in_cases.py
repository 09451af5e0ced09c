"""Crafted streams for the input-rate noise blanker, shared by tests/test_blank_in.py (the numpy twin, no GPU)
and tests/test_gpu_blank_in.py (ft8rx_blank_in* against the twin, bit for bit).  A stream is n = 7 B + 37 samples of one kind: Gaussian
noise from a fixed seed plus planted samples.  Blocks 0 .. 4 carry signal, blocks 5 and 6 are digital silence (L_5 = L_6 = 0: nothing
planted there can hit), block 7 is a tail less than half full (m_7 = 0, L_7 = 0)."""
import numpy as np

from pyft8_amd import blank_in as bi

KINDS = bi.KINDS
KIND_IDS = {bi.REAL_I16: "real_i16", bi.IQ_I16: "iq_i16", bi.WIDE_REAL_I16: "wide_real_i16", bi.WIDE_IQ_I16: "wide_iq_i16",
            bi.WIDE_IQ_U8: "wide_iq_u8", bi.WIDE_IQ_I8: "wide_iq_i8"}
# per dtype: sigma of the noise per component (native units), the magnitude a of a planted hit, the two levels of the tied block
_SCALE = {np.int16: (1000.0, 30000, 500, 700), np.int8: (10.0, 120, 4, 6), np.uint8: (10.0, 250, 8, 12)}


def n_samples(B):
    return 7 * B + 37


def _noise(kind, n, seed):
    dt = bi._DTYPE[kind]
    sigma = _SCALE[dt][0]
    rng = np.random.default_rng(seed)
    v = sigma * rng.standard_normal((n, 2) if bi.is_iq(kind) else n)
    if dt == np.uint8:
        return np.clip(np.rint(127.5 + v), 0, 255).astype(dt)
    info = np.iinfo(dt)
    return np.clip(np.rint(v), info.min + 1, info.max).astype(dt)


def put(x, kind, n, a, sign=1):
    """sample n gets the magnitude a (uint8: a even)"""
    dt = bi._DTYPE[kind]
    if not bi.is_iq(kind):
        x[n] = sign * a
    elif dt == np.uint8:
        assert a % 2 == 0 and 2 <= a <= 256
        x[n] = ((sign * (a - 1) + 255) // 2, 128)
    else:
        x[n] = (sign * a, 0)


def crafted(kind, B, threshold=None, guard=6, taper=6):
    """-> the stream (packed samples of `kind`, n = 7 B + 37) for the parameter set, and the positions planted as hits"""
    B, q8, G, R = bi.check(kind, B, threshold, guard, taper)
    H, n = G + R, n_samples(B)
    dt = bi._DTYPE[kind]
    _, big, t_lo, t_hi = _SCALE[dt]
    x = _noise(kind, n, 1000 + kind)
    # block 1: tied medians -- B / 2 samples of a = t_lo and B / 2 of a = t_hi, so that position B / 2 is the first t_hi
    hi_set = np.flatnonzero(np.random.default_rng(7).permutation(B) >= B // 2) + B
    for i in range(B, 2 * B):
        put(x, kind, i, t_hi if i in set(hi_set.tolist()) else t_lo, -1 if i % 3 == 0 else 1)
    # blocks 3 .. 4: a burst of 1.25 B samples
    for i in range(3 * B + B // 2, 4 * B + 3 * B // 4):
        put(x, kind, i, 2 * (big // 3), -1 if (i * 7) % 5 < 2 else 1)
    # blocks 5, 6: digital silence (uint8: 127 / 128, the smallest magnitude it has)
    x[5 * B:7 * B] = 128 if dt == np.uint8 else 0
    hits = [0, n - 1, 7 * B - 1]                                                      # the first and the last sample, the last full block's end
    hits += [p for b in range(1, 8) for p in (b * B - 1, b * B)]                      # both sides of every block edge
    hits += [p for m in (8 * 5, 64 * 3, 2048, 64 * 2 + 8 * 3) if m < 5 * B for p in (m - 1, m)]   # ... of multiples of 8, 64 (and 2048)
    q1 = 2 * B + 16
    q2 = q1 + 3 * H + 8
    q3 = q2 + 4 * H + 8
    hits += [q1, q1 + 1, q2, q2 + H, q3, q3 + 2 * H + 1]                              # pairs 1, G + R and 2 (G + R) + 1 apart
    hits += [p for b in range(1, 5) for p in (b * B - H - 1, b * B - H)]              # both sides of every release boundary
    hits += [5 * B + 100, 6 * B + 9]                                                  # in the silence: L = 0, no hit
    for i, p in enumerate(hits):
        put(x, kind, p, big, -1 if i % 2 else 1)
    # the extremes of the kind, on samples of block 1 that hold t_hi (m_1 stays)
    e = []
    for p in (int(p) for p in hi_set):        # apart from every hit and from each other, so that the one at the threshold stays ungated
        if all(abs(p - q) > 2 * H + 1 for q in hits + e):
            e.append(p)
    assert len(e) >= 4, "guard + taper too large for this block"
    if dt == np.int16:
        x[e[0]] = -32768
        x[e[1]] = 32767 if not bi.is_iq(kind) else (-32768, -32768)                   # a = 65536
    elif dt == np.int8:
        x[e[0]] = (-128, 127)
        x[e[1]] = (-128, -128)
    else:
        x[e[0]] = (0, 255)
        x[e[1]] = (255, 0)
    # exactly at the threshold (no hit) and one step above it (hit), against the L_1 the stream has so far
    L1 = int(bi.reference(x, kind, B, threshold, guard, taper)[2][1, 1])
    step = 2 if dt == np.uint8 else 1
    at = q8 * L1 // 256 // step * step
    put(x, kind, e[2], at, 1)
    put(x, kind, e[3], at + step, -1)
    lv = bi.reference(x, kind, B, threshold, guard, taper)[2]
    assert int(lv[1, 1]) == L1 and at >= t_hi and 256 * at <= q8 * L1 < 256 * (at + step), (L1, at)
    x.setflags(write=False)
    return x, sorted(set(hits)), (e[2], e[3])


def chunkings(n, B, G, R):
    """name -> chunk lengths that add up to n"""
    def cut(step):
        return [min(step, n - i) for i in range(0, n, step)]
    mix, i, k = [], 0, 0
    pattern = [1, B - 1, 3, B + 1, 2 * B + 5, 7, B]
    while i < n:
        c = min(pattern[k % len(pattern)], n - i)
        mix.append(c)
        i += c
        k += 1
    return {"1": cut(1), "B-1": cut(B - 1), "B": cut(B), "B+1": cut(B + 1), "3B+G+R": cut(3 * B + G + R), "mix": mix, "all": [n]}


_cache = {}


def case(kind, B, threshold=None, guard=6, taper=6):
    """-> (x, twin (y, stats, levels), hits, (at, above)), computed once per parameter set and left unchanged"""
    key = (kind, B, threshold, guard, taper)
    if key not in _cache:
        x, hits, thr = crafted(kind, B, threshold, guard, taper)
        y, stats, lv = bi.reference(x, kind, B, threshold, guard, taper)
        for a in (y, stats, lv):
            a.setflags(write=False)
        _cache[key] = (x, (y, stats, lv), hits, thr)
    return _cache[key]


# ---- the benefit recipe: one FT8 channel in a 240 kHz IQ int16 stream with wideband noise, impulses on single input samples
BENEFIT_RATE, BENEFIT_FRAMES, BENEFIT_SIGNALS, BENEFIT_SNR, BENEFIT_SEED = 240000, (900, 901), 30, (-16, 0), 23
BENEFIT_SIGMA_12K = 31.0        # the channel's own noise per 12 kHz sample after scaling: 1.5 x 45 sigma of the stream fits int16
BENEFIT_WIDE_SIGMA = 40.0 ** 0.5   # wideband noise per component, in units of it: the channel's own noise density over all of 240 kHz
BENEFIT_IMPULSES, BENEFIT_PEAK = 100.0, 45.0
# (The wideband noise is what an SDR band looks like, and what keeps the clean stream Gaussian: a stream that holds little more than
# one 6 kHz channel fades by 15 dB within a few blocks and hits at any sane k.  It costs the channel 3 dB.)
# peak_sigma by the sqrt(rate / 6000) law: the filters take a one-sample impulse down by rate / 6000 = 40 and the noise by sqrt(40),
# so P sigma of the stream arrive at 12 kHz as about P / sqrt(40) = 0.16 P sigma; P = 45 x U[0.5, 1.5] puts the 12 kHz peaks at
# about 3.5 .. 10.5 sigma, on both sides of that blanker's 5.4 sigma, while every one is far above 5.5 medians at the input.


def benefit_recipe():
    """-> list per frame of (clean IQ int16 [3596288, 2], with impulses, f_off, gain, truth = the set of transmitted texts)"""
    if "benefit" not in _cache:
        import ddc_cases
        from pyft8_amd import synth
        rate, n = BENEFIT_RATE, 180000 * (BENEFIT_RATE // 12000)
        rng = np.random.default_rng(BENEFIT_SEED)
        f_off = ddc_cases.offsets(rate)[0]
        out = []
        for i in BENEFIT_FRAMES:
            audio, truth = synth.make_frame(i, n_signals=BENEFIT_SIGNALS, snr_range=BENEFIT_SNR, return_truth=True)
            s = BENEFIT_SIGMA_12K / (float(np.median(np.abs(audio.astype(np.int64)))) / 0.6745)
            spec = np.zeros(n, np.complex128)
            ddc_cases._place(spec, audio, f_off)
            x = np.fft.ifft(spec) * (n / 180000.0) * s
            x += BENEFIT_WIDE_SIGMA * BENEFIT_SIGMA_12K * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
            x = x[:n // 4096 * 4096]          # whole blocks: a tail block that is at least half full has a small m > 0 of its own
            clean = np.clip(np.stack([np.rint(x.real), np.rint(x.imag)], axis=1), -32768, 32767).astype(np.int16)
            noisy = bi.add_impulses(clean, bi.WIDE_IQ_I16, rng, BENEFIT_IMPULSES, rate, BENEFIT_PEAK)
            clean.setflags(write=False)
            noisy.setflags(write=False)
            out.append((clean, noisy, f_off, 1.0 / s, {m["msg"] for m in truth}))
        _cache["benefit"] = out
    return _cache["benefit"]
