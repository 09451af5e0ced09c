"""FT4 (host/numpy, float64): the protocol constants, a synthesiser and the twin of the GPU front end (csrc/kernels/ft4.hpp).

FT4 shares FT8's 77-bit messages, CRC-14 and LDPC(174,91); it differs in front of the decoder: 7.5-s slots, 4-GFSK at 20.8333 baud
(576 samples per symbol at 12 kHz, BT = 1.0), 105 symbols  R S4a D29 S4b D29 S4c D29 S4d R  and a 77-bit scrambling vector that is
XORed onto the message before the CRC and the LDPC code.  The constants are committed as data (QEX 2020 / the WSJT-X generator
tables and the byte table of ft8_lib agree on them; tests/test_ft4.py holds their checks).  No foreign FT4 signal has been decoded
yet: the mode is pinned to these constants and to this twin.

The twin is the definition the kernels are held to (tests/test_gpu_ft4.py):
  grid     P[r][k] = |rfft(hann_periodic(1152) x[144 r : 144 r + 1152])[k]|^2, r = 0 .. 617, k = 0 .. 576 (10.4167 Hz; two bins per
           tone, four rows per symbol), kept as dB = 10 log10(max(P, 1e-24))
  search   score(f0, h0) = sum over the 16 Costas symbols s of dB[tone] - mean dB[other three tones], row h0 + 4 s - 2, columns
           f0 + 2 tone, rows outside the grid contribute 0; per f0 the first strict maximum over h0; kept: best >= sync_min and
           >= both neighbours' best (a tie goes to the lower bin); then the max_cands highest, ties in f0 order
  fine     9 x 5 trials dt = -144 .. 144 step 36 samples, df = -2 .. 2 x 2.6042 Hz: sum over the 16 sync symbols of the magnitude of
           the 576-sample rectangular DFT at the Costas tone, straight from the audio (zeros outside the frame); first maximum in
           (dt, df) order
  demod    the 105 x 4 amplitude matrix at the winner; 174 max-log LLRs on amplitudes (positive = bit 1), scaled 2.83 / std (all
           zero where std = 0; otherwise an LLR of exactly 0 -- a symbol outside the frame -- becomes +0.001); SNR from the
           matrix's powers
and, opt-in, of the coherent LLRs (k_ft4_coh, tests/test_gpu_ft4_coherent.py; coherent_llrs below).  FT4 is
continuous-phase 4-GFSK with tone spacing = baud rate, so consecutive symbols are phase-coherent and runs of symbols can be decided
jointly.  Input: a candidate (f0, h0) with the fine sync's winner (tt, ft); fq = 4 f0 + ft, start = 144 h0 + 36 tt:
  complex  C[s][t] = (sum_{n < 576} x[start + 576 s + n] e^{-2 pi i ((fq + 8 t) n mod 4608) / 4608}) e^{-2 pi i ((fq s) mod 8) / 8},
           s = 0 .. 104, t = 0 .. 3, x = 0 outside the frame.  The first factor is demod's DFT, its phase restarting per symbol; the
           second carries tone 0's phase from symbol to symbol: fq 576 / 4608 turns per symbol is an exact number of eighths, and the
           tones' own 8 t add whole turns.  |C| = amplitudes
  residual for q = -4 .. 4 (quarter steps of 2.6042 Hz): M(q) = sum over the four Costas blocks b of
           |sum_{k < 4} C[p_b + k][costas_b[k]] e^{-2 pi i ((q (p_b + k)) mod 32) / 32}|; the first maximum in the order -4 .. 4; then
           row s of C is multiplied by e^{-2 pi i ((q s) mod 32) / 32}: a rotation per symbol, an exact 32nd of a turn, nothing inside
           a symbol is touched
  runs     symbols 1 .. 103 in runs of L = 2 and L = 4 consecutive symbols from symbol 1 on (the last run is shorter: 1 and 3
           symbols); a sync symbol inside a run enters with its Costas tone, a run without data symbols is skipped; over all 4^d
           assignments of the run's d <= 4 data symbols a = |sum over the run's symbols of C[s][tone_s]|, data tones through GRAY4;
           per bit of the run LLR = max{a : bit = 1} - max{a : bit = 0}
  scaling  as demod: 2.83 / std over the 174 values, all zero where std = 0, otherwise an exact 0 becomes +0.001
L = 1 is demod's LLRs again (tests/test_ft4_coherent.py holds it to 1e-12).
and, opt-in, of the whole-message score behind OSD on those rows (k_ft4_verify, tests/test_gpu_ft4_coh_osd.py; verify_score below;
DESIGN.md section 19.11).  Input: a candidate with its winner (tt, ft), its residual q and a 77-bit word:
  score    C = complex above, row s turned by e^{-2 pi i ((q s) mod 32) / 32}; T = tones105(word); the runs of four symbols from symbol 1
           on, R_k = {1 + 4 k .. min(4 + 4 k, 103)}, k = 0 .. 25 (the last one has three symbols; symbols 0 and 104 never enter):
           A = sum_k |sum_{s in R_k} C[s][T[s]]|,  N = (1 / 412) sum_{s = 1 .. 103} sum_t |C[s][t]|^2,  score = A / sqrt(N), 0 where
           N = 0: a clean signal scores near 206 (103 sqrt(4)), noise against a random word near 26 sqrt(pi) = 46.  The kernel adds
           its float32 amplitudes in float64, every sum in index order
The twin also defines the subtraction passes (csrc/kernels/ft4_sub.hpp, tests/test_gpu_ft4_sub.py; stated in full where sub_model stands, below):
  model    the complex form of tones_to_wave; bins: 41 bins (+-3.97 Hz) of the 60480-point transform of x conj(model); refine: the
           bins' energy at 13 starts 4 samples apart, the first maximum; subtract: x -= 2 Re(a model), a = the bins' inverse transform
and, opt-in, the measured reports (csrc/kernels/ft4_report.hpp, tests/test_gpu_ft4_report.py; stated in full where report stands, below;
DESIGN.md section 19.9): a decoded signal against the same model on a 13 x 13 map of starts and frequencies -> SNR, frequency, time
and, opt-in, the weak search (csrc/kernels/ft4_weak.hpp, tests/test_gpu_ft4_weak.py; weak_sums, weak_score_map
and search_weak below).  It replaces grid and search above and hands the same (f0, h0, score) candidates on.  All phases are exact
integers over 4608; fq is a carrier in units of 12000 / 4608 Hz, r a row (its symbol starts at sample 144 r; r may be negative or run
past the frame, samples outside the frame are zeros), t a tone:
  sums     W[r][fq][t] = sum_{n < 576} x[144 r + n] e^{-2 pi i ((fq (144 r + n) + 8 t n) mod 4608) / 4608}: the carrier's phase is
           referred to sample 0 of the frame, the tone's offset restarts at the symbol, as the transmitted phase does.  For r = h0 + 4 s
           this is C[s][t] above (at tt = 0) up to one constant phase per candidate
  score    for Costas block b with first symbol p_b: B_b(fq, h) = sum_{k < 4} W[h + 4 (p_b + k)][fq][costas_b[k]];
           N(fq, h) = (1 / 64) sum over the 16 sync symbols and the 4 tones of |W|^2;
           score(fq, h) = (|B_0| + |B_1| + |B_2| + |B_3|) / sqrt(N), 0 where N = 0: 0 .. 32, a clean signal on the grid near 32
  per f0   best[f0] = the maximum of score(fq, h) over fq = 4 f0 - 2 .. 4 f0 + 1 (a negative fq is not evaluated) and h in the h0
           range, the first maximum in (fq, h) order, fq ascending then h ascending; h0[f0] is that h; the winner's fq is not handed on
  kept     search's rule with weak_min in place of sync_min, then the max_cands highest, ties in f0 order
The FFT form (weak_grid): G[r][fq'] = W[r][fq'][0] for fq' = 0 .. 2305 serves all four tones, W[r][fq][t] = i^(t r) G[r][fq + 8 t]; per
row it is eight 576-point transforms of the row's samples mixed by fq' mod 8 eighths of a bin, then a turn by (fq' r mod 32) / 32.
"""
import numpy as np

from .ft8_tables import CHK_N, CHK_V
from .synth import encode174, pack77, pack77_ext, random_message        # noqa: F401  (re-exported: the FT4 generator's message side)

FS = 12000
NSPS = 576
NFRAME = 90000
NSYM = 105
NFFT, HOP, ROWS, COLS = 1152, 144, 618, 577
BIN_HZ = FS / NFFT                     # 10.41667
TONE_HZ = FS / NSPS                    # 20.83333
DF_HZ = FS / 4608                      # 2.60417: the fine frequency step
DT_STEP, N_DT, N_DF = 36, 9, 5
COSTAS4 = ((0, 1, 3, 2), (1, 0, 2, 3), (2, 3, 1, 0), (3, 2, 0, 1))
SYNC_POS = (1, 34, 67, 100)
GRAY4 = (0, 1, 3, 2)                   # 2-bit value -> tone
GRAY4_INV = (0, 1, 3, 2)               # tone -> 2-bit value
RVEC_BITS = "0100101001011110100010011011010010110000100010100111100101010101101111100" "0101"
RVEC = int(RVEC_BITS, 2)               # as a 77-bit integer, first transmitted bit = bit 76
SEED_BASE = 0x46543400
SYNC_MIN_DEFAULT = 100.0
OSD_MAX_HD_DEFAULT = 40                # FT8RX_FT4_OSD_MAX_HD_DEFAULT: the largest gate without a false decode on 2048 noise frames
OSD_MAX_HD_MSG_TYPES = 24              # ... and with msg_types = all (one false RTTY-RU word from 28 on): what Receiver takes then
WEAK_MIN_DEFAULT = 16.17               # FT8RX_FT4_WEAK_MIN_DEFAULT
WEAK_NFQ = 4 * NSPS + 2                # carriers of the weak search's grid: fq' = 0 .. 2305 (f0 = 570 reads 4 f0 + 1 + 24)
LLR_SCALE = 2.83
LLR_ZERO = 1e-3                        # what an LLR of exactly 0 becomes: the shared BP's message update divides by tanh(llr / 2)
# symbol index of each of the 87 data symbols, and (symbol, tone) of the 16 sync symbols
DATA_POS = tuple(list(range(5, 34)) + list(range(38, 67)) + list(range(71, 100)))
SYNC_SYMS = tuple((p + s, COSTAS4[b][s]) for b, p in enumerate(SYNC_POS) for s in range(4))


# ----------------------------------------------------------------------------- transmit side
def tones105(bits77):
    """77-bit message -> the 105 tones (0 .. 3) of its FT4 transmission."""
    cw = encode174(int(bits77) ^ RVEC)
    d = [GRAY4[(cw >> (172 - 2 * i)) & 3] for i in range(87)]
    return ([0] + list(COSTAS4[0]) + d[:29] + list(COSTAS4[1]) + d[29:58] + list(COSTAS4[2]) + d[58:] + list(COSTAS4[3]) + [0])


def tones_to_bits77(tones):
    """The inverse of tones105 on an error-free tone list: the descrambled 77-bit message (no CRC check)."""
    cw = 0
    for p in DATA_POS:
        cw = (cw << 2) | GRAY4_INV[int(tones[p])]
    return (cw >> 97) ^ RVEC


def _gfsk_pulse(bt=1.0):
    from math import erf, log, pi, sqrt
    k = pi * sqrt(2.0 / log(2.0)) * bt
    t = (np.arange(3 * NSPS) - 1.5 * NSPS) / NSPS
    return np.array([0.5 * (erf(k * (x + 0.5)) - erf(k * (x - 0.5))) for x in t])


_PULSE = None


def tones_to_wave(tones, f0):
    """105 tones -> the real 4-GFSK waveform, 105 * 576 samples, unit amplitude; f0 = the frequency of tone 0.  The first and the
    last symbol (the ramp symbols) are shaped by a raised cosine over the whole symbol."""
    global _PULSE
    if _PULSE is None:
        _PULSE = _gfsk_pulse()
    n = len(tones)
    ext = [tones[0]] + list(tones) + [tones[-1]]          # dummy edge symbols
    dphi = np.zeros((n + 2) * NSPS + 2 * NSPS)
    for i, t in enumerate(ext):
        dphi[i * NSPS:i * NSPS + 3 * NSPS] += t * _PULSE
    dphi = dphi[2 * NSPS: 2 * NSPS + n * NSPS]
    dphi = 2 * np.pi * (f0 + TONE_HZ * dphi) / FS
    w = np.sin(np.cumsum(dphi) - dphi)
    ramp = 0.5 * (1 - np.cos(np.pi * np.arange(NSPS) / NSPS))
    w[:NSPS] *= ramp
    w[-NSPS:] *= ramp[::-1]
    return w


def amplitude(snr_db):
    """Amplitude (in units of the noise's standard deviation) of a carrier at snr_db in 2500 Hz, synth.make_frame's convention."""
    return np.sqrt(2.0 * (2500.0 / 6000.0) * 10.0 ** (float(snr_db) / 10.0))


def frame_with_signals(index, signals, seed_base=SEED_BASE, noise=True):
    """A 7.5-s frame carrying signals = [(word77, f0 Hz, t0 s, snr dB), ...] at the given places (t0 may be negative or run past
    the end: the part inside the frame is added) -> int16[90000].  Noise: unit variance x 1000 counts, Philox keyed on the index."""
    rng = np.random.Generator(np.random.Philox(key=seed_base + 99000000 + int(index)))
    x = rng.standard_normal(NFRAME) if noise else np.zeros(NFRAME)
    for w77, f0, t0, snr in signals:
        w = tones_to_wave(tones105(int(w77)), float(f0))
        i0 = int(round(float(t0) * FS))
        a, b = max(0, i0), min(NFRAME, i0 + len(w))
        if b > a:
            x[a:b] += amplitude(snr) * w[a - i0:b - i0]
    return np.clip(np.rint(x * 1000.0), -32768, 32767).astype(np.int16)


def make_frame(index, n_signals=6, snr_range=(-8.0, 5.0), seed_base=SEED_BASE, return_truth=False, freq_range=(200.0, 2800.0),
               t0_range=(0.1, 1.5), min_sep_hz=150.0, words=None):
    """One synthetic FT4 frame -> int16[90000] (and the truth list if asked): n_signals standard messages (or the given 77-bit
    `words`), carriers in freq_range at least min_sep_hz apart, starts in t0_range seconds, SNR uniform in snr_range (dB in 2500 Hz)."""
    rng = np.random.Generator(np.random.Philox(key=seed_base + int(index)))
    x = rng.standard_normal(NFRAME)
    truth, used = [], []
    n = len(words) if words is not None else n_signals
    for k in range(n):
        msg = random_message(rng)
        for _ in range(1000):
            f0 = rng.uniform(*freq_range)
            if all(abs(f0 - u) >= min_sep_hz for u in used):
                break
        else:
            raise ValueError("make_frame: the carriers do not fit the range at this separation")
        used.append(f0)
        t0 = rng.uniform(*t0_range)
        snr = rng.uniform(*snr_range)
        w77 = int(words[k]) if words is not None else pack77(*msg)
        w = tones_to_wave(tones105(w77), f0)
        i0 = int(round(t0 * FS))
        m = min(len(w), NFRAME - i0)
        x[i0:i0 + m] += amplitude(snr) * w[:m]
        truth.append(dict(msg=" ".join(msg) if words is None else None, word=w77, f0=float(f0), t0=i0 / FS, snr=float(snr)))
    y = np.clip(np.rint(x * 1000.0), -32768, 32767).astype(np.int16)
    return (y, truth) if return_truth else y


# ----------------------------------------------------------------------------- the twin: grid and search
def hann_periodic(n=NFFT):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def grid_power(x):
    """int16 / float [90000] -> P float64 [618][577]."""
    x = np.asarray(x, np.float64)
    idx = HOP * np.arange(ROWS)[:, None] + np.arange(NFFT)[None, :]
    X = np.fft.rfft(x[idx] * hann_periodic()[None, :], axis=1)
    return X.real ** 2 + X.imag ** 2


def grid_db(P):
    return 10.0 * np.log10(np.maximum(P, 1e-24))


def time_range_to_h0(search_time_range=(-0.5, 2.0)):
    """Absolute start seconds -> (h0_lo, h0_hi), h0_hi exclusive, in rows of 12 ms."""
    lo, hi = search_time_range
    return int(np.rint(lo * FS / HOP)), int(np.rint(hi * FS / HOP)) + 1


def freq_range_to_f0(search_freq_range=(12.5, 5900.0)):
    """Hz -> (f0_lo, f0_hi), f0_hi exclusive, bins of 10.4167 Hz; tone 3 sits 6 bins above f0, so f0_hi <= 571."""
    lo, hi = search_freq_range
    a, b = int(np.ceil(lo / BIN_HZ - 1e-9)), int(np.floor(hi / BIN_HZ + 1e-9)) + 1
    return max(a, 0), min(b, COLS - 6)


def score_map(db, f0_lo, f0_hi, h0_lo, h0_hi, weights=None):
    """score[f0 - f0_lo][h0 - h0_lo] of the search.  weights = (own, other): the factors of the tone's own term and of each of the
    other three (default 1, -1/3; tests bound the score's error with (1, +1/3) on a map of per-bin dB errors)."""
    own, oth = (1.0, -1.0 / 3.0) if weights is None else weights
    f0s, h0s = np.arange(f0_lo, f0_hi), np.arange(h0_lo, h0_hi)
    out = np.zeros((len(f0s), len(h0s)))
    for sym, tone in SYNC_SYMS:
        rows = h0s + 4 * sym - 2
        ok = (rows >= 0) & (rows < ROWS)
        r = np.clip(rows, 0, ROWS - 1)
        t4 = np.stack([db[r][:, f0s + 2 * t] for t in range(4)])           # [4][h0][f0]
        term = own * t4[tone] + oth * (t4.sum(axis=0) - t4[tone])
        out += np.where(ok[:, None], term, 0.0).T
    return out


def _keep(best, h0, f0_lo, floor, max_cands):
    """best [nf0], h0 [nf0] -> the kept candidates [(f0, h0, score), ...]: best >= floor and >= both neighbours' (a tie goes to the lower
    bin), the max_cands highest, ties in f0 order"""
    n = len(best)
    keep = []
    for i in range(n):
        if not best[i] >= floor:
            continue
        if i > 0 and best[i - 1] >= best[i]:
            continue
        if i + 1 < n and best[i + 1] > best[i]:
            continue
        keep.append(i)
    keep.sort(key=lambda i: -best[i])                                      # stable: ties stay in f0 order
    return [(f0_lo + i, int(h0[i]), float(best[i])) for i in keep[:max_cands]]


def search(db, f0_lo, f0_hi, h0_lo, h0_hi, sync_min=SYNC_MIN_DEFAULT, max_cands=200, full=False):
    """-> [(f0, h0, score), ...] in output order (score descending, ties in f0 order); full: also (best[f0], h0[f0], score map)."""
    S = score_map(db, f0_lo, f0_hi, h0_lo, h0_hi)
    bh = np.argmax(S, axis=1)                                              # the first maximum
    best = S[np.arange(len(S)), bh]
    out = _keep(best, h0_lo + bh, f0_lo, sync_min, max_cands)
    return (out, best, h0_lo + bh, S) if full else out


# ----------------------------------------------------------------------------- the twin: weak search (csrc/kernels/ft4_weak.hpp, section 19.10)
def weak_sums(x, rows, fqs):
    """W[len(rows)][len(fqs)][4] of the definition, straight from the samples: every phase an exact integer over 4608."""
    x = np.asarray(x, np.float64)
    rows, fqs = np.asarray(rows, np.int64).reshape(-1), np.asarray(fqs, np.int64).reshape(-1)
    V = _symbols(x, HOP * rows)                                            # [rows][576], zeros outside the frame
    table = np.exp(-2j * np.pi * np.arange(4608) / 4608.0)
    out = np.zeros((len(rows), len(fqs), 4), np.complex128)
    for i, r in enumerate(rows):
        for t in range(4):
            ph = (fqs[:, None] * (HOP * int(r) + _N[None, :]) + 8 * t * _N[None, :]) % 4608
            out[i, :, t] = table[ph] @ V[i]
    return out


def weak_grid(x, r_lo, r_hi):
    """The FFT form: G[r - r_lo][fq'] = W[r][fq'][0], r = r_lo .. r_hi - 1, fq' = 0 .. 2305.  fq' = 8 m + j: the row's samples times
    e^{-2 pi i j n / 4608}, a 576-point transform, bin m, then e^{-2 pi i ((fq' r) mod 32) / 32} for the row's start."""
    x = np.asarray(x, np.float64)
    rows = np.arange(int(r_lo), int(r_hi))
    V = _symbols(x, HOP * rows)
    fq = np.arange(WEAK_NFQ)
    G = np.zeros((len(rows), WEAK_NFQ), np.complex128)
    for j in range(8):
        Z = np.fft.fft(V * np.exp(-2j * np.pi * (j * _N) / 4608.0)[None, :], axis=1)
        sel = fq[fq % 8 == j]
        G[:, sel] = Z[:, sel // 8]
    return G * np.exp(-2j * np.pi * ((fq[None, :] * rows[:, None]) % 32) / 32.0)


def _weak_terms(G, r_lo, fq_lo, fq_hi, h0_lo, h0_hi):
    """-> (B [4][fq][h] the block sums, E [fq][h] = sum of |W|^2 over the 16 sync symbols and 4 tones) on the grid G of rows r_lo .."""
    fqs, hs = np.arange(fq_lo, fq_hi), np.arange(h0_lo, h0_hi)
    B = np.zeros((4, len(fqs), len(hs)), np.complex128)
    E = np.zeros((len(fqs), len(hs)))
    for sym, tone in SYNC_SYMS:
        b = SYNC_POS.index(sym - (sym - 1) % 33)
        r = hs + 4 * sym
        for t in range(4):
            g = G[(r - r_lo)[None, :], (fqs + 8 * t)[:, None]]             # [fq][h]
            E += g.real ** 2 + g.imag ** 2
            if t == tone:
                B[b] += g * (1j ** ((t * r) % 4))[None, :]                  # an exact quarter-turn power
    return B, E


def weak_score_map(x, fq_lo, fq_hi, h0_lo, h0_hi, full=False):
    """score[fq - fq_lo][h - h0_lo] of the weak search; fq_lo >= 0.  full: also (S = sum of the four |B_b|, nrm = sqrt(64 N)) --
    score = 8 S / nrm -- for the tests' error bound."""
    G = weak_grid(x, h0_lo + 4, h0_hi + 4 * (NSYM - 2))                     # rows h0_lo + 4 .. h0_hi - 1 + 412
    B, E = _weak_terms(G, h0_lo + 4, fq_lo, fq_hi, h0_lo, h0_hi)
    S, nrm = np.abs(B).sum(axis=0), np.sqrt(E)
    score = np.where(E > 0, 8.0 * S / np.where(E > 0, nrm, 1.0), 0.0)
    return (score, S, nrm) if full else score


def weak_best(score, fq_lo, f0_lo, f0_hi, h0_lo):
    """The per-f0 step on a score map whose first row is carrier fq_lo: -> (best [nf0], h0 [nf0]), the first maximum in (fq, h) order
    over fq = 4 f0 - 2 .. 4 f0 + 1, a negative fq left out."""
    best, bh = np.zeros(f0_hi - f0_lo), np.zeros(f0_hi - f0_lo, np.int64)
    for i, f0 in enumerate(range(f0_lo, f0_hi)):
        a = max(4 * f0 - 2, 0) - fq_lo
        blk = score[a:4 * f0 + 2 - fq_lo]
        k = int(np.argmax(blk))                                             # C order: fq ascending, then h ascending
        best[i], bh[i] = blk.flat[k], h0_lo + k % blk.shape[1]
    return best, bh


def search_weak(x, f0_lo, f0_hi, h0_lo, h0_hi, weak_min=WEAK_MIN_DEFAULT, max_cands=200, full=False):
    """The weak search on one frame -> [(f0, h0, score), ...] in output order; full: also (best [nf0], h0 [nf0], score map, fq_lo)."""
    fq_lo = max(4 * f0_lo - 2, 0)
    S = weak_score_map(x, fq_lo, 4 * (f0_hi - 1) + 2, h0_lo, h0_hi)
    best, bh = weak_best(S, fq_lo, f0_lo, f0_hi, h0_lo)
    out = _keep(best, bh, f0_lo, weak_min, max_cands)
    return (out, best, bh, S, fq_lo) if full else out


# ----------------------------------------------------------------------------- the twin: fine sync and demodulation
_N = np.arange(NSPS)


def _symbols(x, starts):
    """The 576 samples from each of `starts` on, zeros outside x -> [len(starts)][576]."""
    i = np.asarray(starts)[:, None] + _N[None, :]
    ok = (i >= 0) & (i < len(x))
    return np.where(ok, x[np.clip(i, 0, len(x) - 1)], 0.0)


def _phasors(fq):
    """e^(-2 pi i (fq n mod 4608) / 4608), n < 576, for each frequency fq (x 12000 / 4608 Hz) -> [len(fq)][576]: the 576-sample
    rectangular DFT's kernel, the phase restarting at the symbol's first sample."""
    return np.exp(-2j * np.pi * ((np.asarray(fq)[:, None] * _N[None, :]) % 4608) / 4608.0)


def fine_metrics(x, f0, h0):
    """The 9 x 5 sync metrics of candidate (f0 bin, h0 row), [dt index][df index]."""
    x = np.asarray(x, np.float64)
    syms = np.array([s for s, _ in SYNC_SYMS])
    tones = np.array([t for _, t in SYNC_SYMS])
    m = np.zeros((N_DT, N_DF))
    for a in range(N_DT):
        V = _symbols(x, HOP * h0 + DT_STEP * (a - N_DT // 2) + NSPS * syms)
        for b in range(N_DF):
            m[a, b] = np.abs((V * _phasors(4 * f0 + (b - N_DF // 2) + 8 * tones)).sum(axis=1)).sum()
    return m


def amplitudes(x, f0, h0, tt, ft):
    """The 105 x 4 amplitude matrix at time tweak tt (x 36 samples) and frequency tweak ft (x 2.6042 Hz)."""
    x = np.asarray(x, np.float64)
    V = _symbols(x, HOP * h0 + DT_STEP * tt + NSPS * np.arange(NSYM))
    return np.abs(V @ _phasors(4 * f0 + ft + 8 * np.arange(4)).T)


def llr_from_amplitudes(A):
    """174 max-log LLRs (positive = bit 1) of the 87 data symbols, scaled to 2.83 / std; all zero where std is 0, otherwise no LLR is
    exactly 0: the BP behind it (the reference's update, e / ((e - 1.18)(e + 1.18)) with e = P / t) turns a zero into NaNs."""
    D = A[list(DATA_POS)]
    msb = np.maximum(D[:, 2], D[:, 3]) - np.maximum(D[:, 0], D[:, 1])       # tones 2, 3 carry values 3, 2
    lsb = np.maximum(D[:, 1], D[:, 2]) - np.maximum(D[:, 0], D[:, 3])       # tones 1, 2 carry values 1, 3
    return _scale_llrs(np.stack([msb, lsb], axis=1).reshape(174))


def _scale_llrs(llr):
    """174 raw differences -> 2.83 / std of them; all zero where std is 0, otherwise an exact 0 becomes +0.001."""
    sd = np.std(llr)
    if not sd > 0:
        return np.zeros(174)
    llr = LLR_SCALE * llr / sd
    llr[llr == 0.0] = LLR_ZERO                                              # a symbol outside the frame, or in digital silence
    return llr


def snr_from_amplitudes(A):
    """The report: 10 log10((S - N) / N) - 10 log10(2500 / 20.8333), rounded, clipped to +-24 (-24 where S <= N or N = 0)."""
    P = A * A
    top = P.max(axis=1)
    S, N = top.mean(), ((P.sum(axis=1) - top) / 3.0).mean()
    if not (N > 0 and S > N):
        return -24
    return int(np.clip(np.rint(10.0 * np.log10((S - N) / N) - 10.0 * np.log10(2500.0 / TONE_HZ)), -24, 24))


def demod(x, f0, h0):
    """Fine sync and demodulation of one candidate -> dict(tt, ft, metric, metrics, llr, snr, amps)."""
    m = fine_metrics(x, f0, h0)
    k = int(np.argmax(m))                                                  # first maximum in (dt, df) order
    tt, ft = k // N_DF - N_DT // 2, k % N_DF - N_DF // 2
    A = amplitudes(x, f0, h0, tt, ft)
    return dict(tt=tt, ft=ft, metric=float(m.flat[k]), metrics=m, llr=llr_from_amplitudes(A), snr=snr_from_amplitudes(A), amps=A)


# ----------------------------------------------------------------------------- the twin: coherent LLRs (k_ft4_coh)
COH_Q = tuple(range(-4, 5))            # the residual-frequency trials, x 12000 / (32 x 576) = 0.6510 Hz: a 32nd of a turn per symbol
_SYNC_TONE = dict(SYNC_SYMS)
_DATA_INDEX = {p: i for i, p in enumerate(DATA_POS)}


def complex_amplitudes(x, f0, h0, tt, ft):
    """C[105][4] of the definition's step 1: the rectangular DFT of `amplitudes`, kept complex, times the phase tone 0 has gathered
    since symbol 0 -- (fq s mod 8) / 8 of a turn, fq = 4 f0 + ft.  |C| is `amplitudes`."""
    x = np.asarray(x, np.float64)
    fq = 4 * int(f0) + int(ft)
    V = _symbols(x, HOP * int(h0) + DT_STEP * int(tt) + NSPS * np.arange(NSYM))
    C = V @ _phasors(fq + 8 * np.arange(4)).T
    return C * np.exp(-2j * np.pi * ((fq * np.arange(NSYM)) % 8) / 8.0)[:, None]


def coherent_metrics(C):
    """M(q), q = -4 .. 4: per Costas block the magnitude of the four sync symbols' sum, each turned back by (q s mod 32) / 32 of a
    turn; the four blocks' magnitudes added."""
    m = np.zeros(len(COH_Q))
    for i, q in enumerate(COH_Q):
        for b, p in enumerate(SYNC_POS):
            m[i] += abs(sum(C[p + k][COSTAS4[b][k]] * np.exp(-2j * np.pi * ((q * (p + k)) % 32) / 32.0) for k in range(4)))
    return m


def run_llrs(C, L):
    """The 174 scaled LLRs of runs of L symbols (1, 2 or 4) on the complex amplitudes C: symbols 1 .. 103 in runs from symbol 1 on (the
    last one shorter), a sync symbol with its Costas tone, the d data symbols of a run over all 4^d assignments through GRAY4:
    a = |sum of the run's C[s][tone]|, and per bit max{a : bit = 1} - max{a : bit = 0}.  A run without data symbols is skipped."""
    llr = np.zeros(174)
    gray = list(GRAY4)
    for s0 in range(1, NSYM - 1, L):
        syms = range(s0, min(s0 + L, NSYM - 1))
        data = [s for s in syms if s in _DATA_INDEX]
        if not data:
            continue
        acc = np.asarray(sum(C[s][_SYNC_TONE[s]] for s in syms if s in _SYNC_TONE) + 0j)
        for s in data:
            acc = np.add.outer(acc, C[s][gray])                             # one axis per data symbol, indexed by its 2-bit value
        a = np.abs(acc)
        for k, s in enumerate(data):
            v = np.moveaxis(a, k, 0).reshape(4, -1).max(axis=1)             # the best assignment of the others, per value of this symbol
            llr[2 * _DATA_INDEX[s]] = max(v[2], v[3]) - max(v[0], v[1])
            llr[2 * _DATA_INDEX[s] + 1] = max(v[1], v[3]) - max(v[0], v[2])
    return _scale_llrs(llr)


def coherent_llrs(x, f0, h0, tt, ft):
    """Coherent LLRs of candidate (f0, h0) at the fine sync's winner (tt, ft) -> dict(q, metrics[9], llr1, llr2, llr4): the residual
    frequency q (the first maximum of the metrics in the order -4 .. 4), and the LLRs of runs of 1, 2 and 4 symbols on the complex
    amplitudes turned back by (q s mod 32) / 32 of a turn per symbol.  llr1 is llr_from_amplitudes(amplitudes(...)) again: a
    rotation leaves a single symbol's magnitudes alone."""
    C = complex_amplitudes(x, f0, h0, tt, ft)
    m = coherent_metrics(C)
    q = COH_Q[int(np.argmax(m))]
    C = C * np.exp(-2j * np.pi * ((q * np.arange(NSYM)) % 32) / 32.0)[:, None]
    return dict(q=q, metrics=m, llr1=run_llrs(C, 1), llr2=run_llrs(C, 2), llr4=run_llrs(C, 4))


# ----------------------------------------------------------------------------- the twin: the whole-message score (k_ft4_verify, section 19.11)
COH_OSD_MIN_SCORE_DEFAULT = 77.1       # FT8RX_FT4_COH_OSD_MIN_SCORE_DEFAULT: measured on the noise words within max_hd
COH_OSD_MIN_SCORE_MSG_TYPES = 81.0     # ... and on those at msg_types = all: what Receiver takes then (the rule of OSD_MAX_HD_MSG_TYPES)
COH_OSD_MAX_HD_DEFAULT = 40            # FT8RX_FT4_COH_OSD_MAX_HD_DEFAULT: keeps 99 % of the true words measured (hd 17 .. 39)
VERIFY_RUNS = tuple(range(1, NSYM - 1, 4))      # first symbols of the 26 runs of four


def verify_terms(C, tones):
    """(A, N) of the score's definition on complex amplitudes C [105][4] that are already turned by q."""
    C, T = np.asarray(C), np.asarray(tones, np.int64)
    own = C[np.arange(NSYM), T]
    A = sum(abs(own[s0:min(s0 + 4, NSYM - 1)].sum()) for s0 in VERIFY_RUNS)
    N = float((np.abs(C[1:NSYM - 1]) ** 2).sum()) / 412.0
    return float(A), N


def verify_score(x, f0, h0, tt, ft, q, word77):
    """The whole-message coherent score of the 77-bit word `word77` on candidate (f0, h0) at the fine sync's winner (tt, ft) and the
    residual frequency q of coherent_llrs: A / sqrt(N) of the module's definition, 0 where N = 0."""
    C = complex_amplitudes(x, f0, h0, tt, ft) * np.exp(-2j * np.pi * ((int(q) * np.arange(NSYM)) % 32) / 32.0)[:, None]
    A, N = verify_terms(C, tones105(word77))
    return A / np.sqrt(N) if N > 0 else 0.0


def early_ok(h0_idx, ttweak, n_have):
    """The early-pass rule of live FT4: a decode of a slot of which only the first n_have samples exist is
    delivered iff its whole signal -- start 144 h0 + 36 tt (it may be negative), 105 symbols of 576 samples -- with the fine sync's
    reach of +-4 steps of 36 samples lies inside them.  The fine sync and the demodulator read the signal's own samples only, so such
    a candidate sees the audio it sees in the complete slot."""
    return HOP * int(h0_idx) + DT_STEP * int(ttweak) + NSYM * NSPS + DT_STEP * (N_DT // 2) <= int(n_have)


# ----------------------------------------------------------------------------- message dicts of the GPU path (Receiver.decode_frames_ft4)
def slot_parity(cyclestart_string):
    """'YYMMDD_HHMMSS' (the seconds may carry a fraction: '..._000007.5') -> 0 / 1, the parity of the 7.5-s slot that starts then."""
    try:
        t = cyclestart_string.split("_")[1]
        sec = int(t[0:2]) * 3600 + int(t[2:4]) * 60 + float(t[4:])
    except (IndexError, ValueError):
        return 0
    return int(sec // 7.5) % 2


def message_dicts(msgs, count, cyclestart_string="", band=None, on_message=None, nsym=None, reports=None):
    """Rows of the native packager (ft8rx_package_batch / _ext on FT4 records) -> message dicts with the keys of the FT8 ones and FT4's
    values: tsec = (144 h0 + 36 tt) / 12000, fHz = 10.41667 f0 + 2.60417 ft, "mode": "FT4", '+' in all_txt_format, their_tx_cycle =
    the slot's parity.  nsym (a receiver with ft4_coherent): per row the run length of its decode -> "nsym": 1, 2 or 4.  reports (a
    receiver with ft4_reports; REPORT_DTYPE rows, one per message): "report": {"snr", "fHz", "tsec"}, or None where it is INVALID."""
    import time
    from . import messages as _m
    out = []
    now = time.time()
    rows = msgs[:min(int(count), len(msgs))]
    ext = len(rows) > 0 and "i3" in rows.dtype.names
    parity = slot_parity(cyclestart_string)
    for k, r in enumerate(rows):
        text = tuple(x.decode() for x in r["f"].tolist())
        tt, ft = int(r["ttweak"]), int(r["ftweak"])
        tsec = (HOP * int(r["h0_idx"]) + DT_STEP * tt) / FS
        fHz = BIN_HZ * int(r["f0_idx"]) + DF_HZ * ft
        snr = "%+03d" % int(r["snr"])
        rec = {"ipass": int(r["ipass"]), "method": int(r["method"]), "ap": int(r["ap"]), "ttweak": tt, "ftweak": ft}
        notes, tw = _m.decode_notes(rec)
        word_type = (int(r["i3"]) | (int(r["n3"]) << 3)) if ext else 1
        line = _m._msg_text(word_type, text) if ext else " ".join(text)
        d = {"band": band, "tsec": tsec, "fHz": fHz, "msg_tuple": text, "their_snr": snr, "their_tx_cycle": parity,
             "all_txt_format": f"{cyclestart_string} {snr} {(tsec - 0.5):4.1f} {fHz:4.0f} + {line}",
             "cyclestart_string": cyclestart_string, "decode_completed": now, "tweaks": tw, "decode_notes": notes + tw, "mode": "FT4"}
        if ext:
            d["msg_type"] = _m.msg_type(word_type)
        if nsym is not None:
            d["nsym"] = int(nsym[k])
        if reports is not None:
            p = reports[k]
            ok = (int(p["flags"]) & (RP_MEASURED | RP_INVALID)) == RP_MEASURED
            d["report"] = {"snr": float(p["snr_db"]), "fHz": float(p["f_hz"]), "tsec": float(p["t_sec"])} if ok else None
        out.append(d)
        if on_message is not None:
            on_message(d)
    return out


# ----------------------------------------------------------------------------- a plain sum-product decoder (CPU check of a fixture)
def crc14_ok(bits91):
    from .synth import crc14
    v = int("".join(str(int(b)) for b in bits91), 2)
    return crc14(v >> 14) == (v & 0x3FFF)


def bp_decode(llr, max_iters=50):
    """Sum-product BP on LDPC(174,91) (llr > 0 = bit 1) -> the descrambled 77-bit message, or None.  Shows on the CPU that a fixture
    is decodable; it is not held to the GPU's decoder."""
    chk = [np.array(CHK_V[c][:CHK_N[c]]) for c in range(83)]
    L = np.asarray(llr, np.float64)
    msg = [np.zeros(len(c)) for c in chk]                                  # check -> variable
    for _ in range(max_iters):
        tot = L.copy()
        for c, m in zip(chk, msg):
            np.add.at(tot, c, m)
        hard = tot > 0
        if all(hard[c].sum() % 2 == 0 for c in chk):
            if crc14_ok(hard[:91]):
                return (int("".join("1" if b else "0" for b in hard[:77]), 2)) ^ RVEC
            return None
        for i, c in enumerate(chk):
            t = np.tanh(np.clip(-(tot[c] - msg[i]) / 2.0, -19.0, 19.0))
            prod = np.array([np.prod(np.delete(t, j)) for j in range(len(c))])
            msg[i] = -2.0 * np.arctanh(np.clip(prod, -0.999999999999, 0.999999999999))
    return None


def decode_twin(x, f0_lo=None, f0_hi=None, h0_lo=None, h0_hi=None, sync_min=SYNC_MIN_DEFAULT, max_cands=200, weak=False, weak_min=WEAK_MIN_DEFAULT):
    """The whole twin on one frame: search (weak: search_weak at weak_min instead), fine sync, demodulation, BP
    -> [dict(f0, h0, tt, ft, snr, word or None), ...]."""
    a, b = freq_range_to_f0()
    c, d = time_range_to_h0()
    f0_lo, f0_hi = (a if f0_lo is None else f0_lo), (b if f0_hi is None else f0_hi)
    h0_lo, h0_hi = (c if h0_lo is None else h0_lo), (d if h0_hi is None else h0_hi)
    out = []
    cands = (search_weak(x, f0_lo, f0_hi, h0_lo, h0_hi, weak_min, max_cands) if weak else
             search(grid_db(grid_power(x)), f0_lo, f0_hi, h0_lo, h0_hi, sync_min, max_cands))
    for f0, h0, score in cands:
        r = demod(x, f0, h0)
        out.append(dict(f0=f0, h0=h0, score=score, tt=r["tt"], ft=r["ft"], snr=r["snr"], llr=r["llr"], word=bp_decode(r["llr"])))
    return out


# ----------------------------------------------------------------------------- the twin: subtraction passes (csrc/kernels/ft4_sub.hpp)
# A decoded signal is (start sample s0 = 144 h0 + 36 tt, possibly negative; fq = 4 f0 + ft, tone 0 in units of 12000 / 4608 Hz; the
# 105 tones).  model s[n], n < 60480: the complex form of tones_to_wave.  Analysis y[n] = x[s0 + n] conj(s[n]) (x = 0 outside the
# frame), A[k] = sum_n y[n] e^{-2 pi i k n / 60480}, k = -20 .. 20: a +-3.97-Hz low-pass, wide enough for the +-1.3 Hz the fine grid
# leaves.  Subtraction x[s0 + n] -= 2 Re(a[n] s[n]), a = the inverse transform of the 41 kept bins.  Refine: E(d) = sum_k |A_d[k]|^2
# with the start at s0 + d for d = -24, -20 .. 24; the first maximum wins.  DESIGN.md section 19.6.
SUB_N = NSYM * NSPS                    # 60480 model samples
SUB_K = 20                             # bins -20 .. +20 of 12000 / 60480 = 0.198 Hz
SUB_SHIFTS = tuple(range(-24, 25, 4))  # the 13 refine trials, samples


def sig_from_record(f0, h0, tt, ft, word):
    """(f0 bin, h0 row, time tweak, frequency tweak, 77-bit word) -> dict(start, fq, tones): what a subtraction sweep takes."""
    return dict(start=HOP * int(h0) + DT_STEP * int(tt), fq=4 * int(f0) + int(ft), tones=tones105(int(word)), word=int(word))


def sub_model(tones, fq):
    """The complex model s[60480] of a signal with tone 0 at fq x 12000 / 4608 Hz: Im s = tones_to_wave(tones, fq * DF_HZ)."""
    global _PULSE
    if _PULSE is None:
        _PULSE = _gfsk_pulse()
    n = len(tones)
    ext = [tones[0]] + list(tones) + [tones[-1]]
    dphi = np.zeros((n + 2) * NSPS + 2 * NSPS)
    for i, t in enumerate(ext):
        dphi[i * NSPS:i * NSPS + 3 * NSPS] += t * _PULSE
    dphi = dphi[2 * NSPS: 2 * NSPS + n * NSPS]
    dphi = 2 * np.pi * (fq * 12000.0 / 4608.0 + TONE_HZ * dphi) / FS
    s = np.exp(1j * (np.cumsum(dphi) - dphi))
    ramp = 0.5 * (1 - np.cos(np.pi * np.arange(NSPS) / NSPS))
    s[:NSPS] *= ramp
    s[-NSPS:] *= ramp[::-1]
    return s


def _sub_window(x, s0, n=SUB_N):
    """x[s0 : s0 + n] with zeros outside the frame, and the mask of the samples inside."""
    i = int(s0) + np.arange(n)
    ok = (i >= 0) & (i < len(x))
    return np.where(ok, x[np.clip(i, 0, len(x) - 1)], 0.0), ok


def sub_bins(x, s0, model):
    """The 41 bins A[k], k = -20 .. 20 (index k + 20), of y[n] = x[s0 + n] conj(model[n])."""
    w, _ = _sub_window(np.asarray(x, np.float64), s0, len(model))
    Y = np.fft.fft(w * np.conj(model))
    return np.concatenate([Y[-SUB_K:], Y[:SUB_K + 1]])


def sub_energies(x, s0, model):
    """E(d) of the 13 refine trials around s0."""
    return np.array([(np.abs(sub_bins(x, s0 + d, model)) ** 2).sum() for d in SUB_SHIFTS])


def sub_refine(x, sig, model=None):
    """-> (the refined start: s0 + the first maximum's shift, the 13 energies)."""
    model = sub_model(sig["tones"], sig["fq"]) if model is None else model
    E = sub_energies(x, sig["start"], model)
    return int(sig["start"]) + SUB_SHIFTS[int(np.argmax(E))], E


def sub_apply(x, s0, model):
    """Subtracts the signal at start s0 from the float64 frame x in place; samples outside the frame are never touched."""
    A = sub_bins(x, s0, model)
    S = np.zeros(len(model), np.complex128)
    S[-SUB_K:] = A[:SUB_K]
    S[:SUB_K + 1] = A[SUB_K:]
    a = np.fft.ifft(S)
    i = int(s0) + np.arange(len(model))
    ok = (i >= 0) & (i < len(x))
    x[i[ok]] -= 2.0 * (a * model).real[ok]


def subtract(x, sigs, refine=1):
    """Subtracts sigs (dicts of start, fq, tones) from the float64 frame x in list order, in place -> the starts used."""
    starts = []
    for sg in sigs:
        model = sub_model(sg["tones"], sg["fq"])
        s0 = sub_refine(x, sg, model)[0] if refine else int(sg["start"])
        sub_apply(x, s0, model)
        starts.append(s0)
    return starts


def subtraction_list(decodes, have=()):
    """decodes: (f0, h0, tt, ft, word) in emit order -> the sweep's list: each word once, at its first occurrence, none of `have`."""
    seen, out = set(int(w) for w in have), []
    for f0, h0, tt, ft, word in decodes:
        if int(word) in seen:
            continue
        seen.add(int(word))
        out.append(sig_from_record(f0, h0, tt, ft, word))
    return out


_CHK_IDX = None


def bp_decode_many(llrs, max_iters=50):
    """bp_decode on rows of LLRs at once (the same sum-product update and stopping rule, vectorised) -> [word or None, ...]."""
    global _CHK_IDX
    L = np.atleast_2d(np.asarray(llrs, np.float64))
    if _CHK_IDX is None:
        idx = np.full((83, 7), 174, np.int64)                              # column 174: a dummy variable that is never wrong
        for c in range(83):
            idx[c, :CHK_N[c]] = CHK_V[c][:CHK_N[c]]
        _CHK_IDX = idx
    idx, pad = _CHK_IDX, _CHK_IDX == 174
    n = len(L)
    out = [None] * n
    live = np.arange(n)
    msg = np.zeros((n, 83, 7))
    for _ in range(max_iters):
        if len(live) == 0:
            break
        tot = np.concatenate([L[live], np.zeros((len(live), 1))], axis=1)
        np.add.at(tot, (np.arange(len(live))[:, None, None], idx[None]), np.where(pad, 0.0, msg[live]))
        hard = tot[:, :174] > 0
        h7 = np.where(pad, False, np.concatenate([hard, np.zeros((len(live), 1), bool)], axis=1)[:, idx])
        done = (h7.sum(axis=2) % 2 == 0).all(axis=1)
        for j in np.nonzero(done)[0]:
            if crc14_ok(hard[j, :91]):
                out[live[j]] = int("".join("1" if b else "0" for b in hard[j, :77]), 2) ^ RVEC
        keep = ~done
        t = np.tanh(np.clip(-(tot[keep][:, idx] - msg[live[keep]]) / 2.0, -19.0, 19.0))
        t = np.where(pad, 1.0, t)
        prod = np.stack([np.prod(np.delete(t, j, axis=2), axis=2) for j in range(7)], axis=2)
        live = live[keep]
        msg[live] = np.where(pad, 0.0, -2.0 * np.arctanh(np.clip(prod, -0.999999999999, 0.999999999999)))
    return out


def decode_twin_passes(x, passes=2, max_cands=200, sync_min=SYNC_MIN_DEFAULT, refine=1):
    """decode_twin with subtraction passes on one int16 frame -> [dict(start, fq, word, pass), ...], the words in emit order
    (score order within a pass), each once.  Pass p + 1: subtract the words new since pass p from a float copy, round it back to int16
    (rint, clipped), decode again, append the words the frame does not have yet; stops when a pass brings nothing new."""
    a, b = freq_range_to_f0()
    c, d = time_range_to_h0()
    work = np.asarray(x, np.float64).copy()
    cur = np.asarray(x, np.int16)
    out, have, fresh = [], set(), []
    for p in range(int(passes)):
        if p:
            if not fresh:
                break
            subtract(work, fresh, refine)
            cur = np.clip(np.rint(work), -32768, 32767).astype(np.int16)
            work = cur.astype(np.float64)
        cands = search(grid_db(grid_power(cur)), a, b, c, d, sync_min, max_cands)
        dem = [demod(cur, f0, h0) for f0, h0, _ in cands]
        words = bp_decode_many([r["llr"] for r in dem]) if dem else []
        dec = [(f0, h0, r["tt"], r["ft"], w) for (f0, h0, _), r, w in zip(cands, dem, words) if w is not None]
        fresh = subtraction_list(dec, have)
        for sg in fresh:
            have.add(sg["word"])
            out.append({"start": sg["start"], "fq": sg["fq"], "word": sg["word"], "pass": p + 1})
    return out


# ----------------------------------------------------------------------------- the twin: measured reports (csrc/kernels/ft4_report.hpp)
# Once a signal has decoded its 105 tones are known, and it can be measured against its own model.  With the
# model s = sub_model(tones, fq), trial starts s0 + tau (tau = -36, -30 .. 36) and y_tau[n] = x[s0 + tau + n] conj(s[n]) (x = 0
# outside [0, n_have)), everything is defined on the segment sums G_tau[j] = sum_{n < 36} y_tau[36 j + n], j < 1680:
#   score    C_tau,delta[q] = sum_{j < 16} G_tau[16 q + j] e^{-2 pi i delta (36 (16 q + j) + 17.5) / 12000}, delta = -6 .. 6 steps of
#            0.6510 Hz; P(tau, delta) = sum over the blocks {1..4}, {5..8} .. {97..100}, {101..103} of |sum_{q in block} C[q]|^2
#   peak     the first maximum in tau-major order; a three-point parabola on each axis where the peak is interior (a zero denominator
#            gives 0), else RP_EDGE_T / RP_EDGE_F; t_sec = (s0 + tau + 6 dt) / 12000, f_hz = fq 12000 / 4608 + delta, score = P there
#   SNR      at the peak's tau and the interpolated delta, over the valid symbols (q = 1 .. 103 whose 576 samples lie inside
#            [0, n_have); fewer than RP_MIN_VALID: RP_INVALID, NaN fields): on = mean |C[q]|^2; off = the lower quartile of the
#            Hann-weighted cells of the same samples at fq + 8 t, t in RP_CELLS (a frequency outside [8, 2296] is dropped whole),
#            c[(m - 1) // 4] / ln(4 / 3) x 576 / 216; snr_db = 10 log10(max(on / off - 1, 1e-3) x 20.8333 / 2500), off = 0: the floor
RP_MEASURED, RP_INVALID, RP_EDGE_T, RP_EDGE_F = 1, 2, 4, 8            # FT8RX_RP_*
RP_TAUS = tuple(range(-36, 37, 6))     # the 13 trial starts, samples
RP_DELTAS = tuple(range(-6, 7))        # the 13 trial frequencies, x RP_DELTA_HZ
RP_DELTA_HZ = FS / 4608 / 4            # 0.6510 Hz: k_ft4_coh's step
RP_SEG = 36                            # samples per segment sum: 16 segments per symbol
RP_BLOCK = 4                           # symbols summed coherently
RP_CELLS = (-5, -4, -3, 6, 7, 8)       # the noise cells, in tones from tone 0
RP_FQ_LO, RP_FQ_HI = 8, 2296           # a cell frequency outside (x 2.6042 Hz) is dropped
RP_MIN_VALID = 32
RP_SNR_FLOOR = 1e-3
RP_HANN_SUM2 = 216.0                   # sum w^2 of w[n] = 1/2 - 1/2 cos(2 pi (n + 1/2) / 576)


def report_segments(x, s0, model, n_have=NFRAME):
    """G_tau[1680] of y[n] = x[s0 + n] conj(model[n]), x = 0 outside [0, n_have)."""
    x = np.asarray(x, np.float64)[:int(n_have)]
    w, _ = _sub_window(x, s0, len(model))
    return (w * np.conj(model)).reshape(-1, RP_SEG).sum(axis=1)


def report_symbols(G, delta_steps):
    """C[105] of the segment sums at the frequency offset delta_steps x 0.6510 Hz (a float: the interpolated peak)."""
    j = np.arange(len(G))
    ph = np.exp(-2j * np.pi * (float(delta_steps) * RP_DELTA_HZ) * (RP_SEG * j + 17.5) / FS)
    return (G * ph).reshape(NSYM, NSPS // RP_SEG).sum(axis=1)


def report_score(C):
    """P of one (tau, delta): symbols 1 .. 103 in blocks of four from symbol 1 on, coherent inside a block."""
    return float(sum(abs(C[a:min(a + RP_BLOCK, NSYM - 1)].sum()) ** 2 for a in range(1, NSYM - 1, RP_BLOCK)))


def _parabola(a, b, c):
    den = a - 2.0 * b + c
    return 0.5 * (a - c) / den if den != 0.0 else 0.0


def report(x, sig, n_have=NFRAME, full=False):
    """The measured report of one decoded signal (sig_from_record's dict) on the frame x -> dict(flags, snr_db, f_hz, t_sec, score; the
    four are NaN with RP_INVALID), and the stages: scores [13][13], on, off, tau, delta (steps, interpolated), n_valid; full: also
    cells, the sorted cell powers."""
    x = np.asarray(x, np.float64)
    n_have = int(n_have)
    s0, fq = int(sig["start"]), int(sig["fq"])
    model = sub_model(sig["tones"], fq)
    G = [report_segments(x, s0 + tau, model, n_have) for tau in RP_TAUS]
    P = np.array([[report_score(report_symbols(g, d)) for d in RP_DELTAS] for g in G])
    k = int(np.argmax(P))                                                  # the first maximum in tau-major order
    it, idl = divmod(k, len(RP_DELTAS))
    flags, dt, dd = RP_MEASURED, 0.0, 0.0
    if 0 < it < len(RP_TAUS) - 1:
        dt = _parabola(P[it - 1, idl], P[it, idl], P[it + 1, idl])
    else:
        flags |= RP_EDGE_T
    if 0 < idl < len(RP_DELTAS) - 1:
        dd = _parabola(P[it, idl - 1], P[it, idl], P[it, idl + 1])
    else:
        flags |= RP_EDGE_F
    tau, delta = RP_TAUS[it], RP_DELTAS[idl] + dd
    out = dict(scores=P, tau=tau, delta=delta, score=float(P[it, idl]))
    starts = s0 + tau + NSPS * np.arange(NSYM)
    valid = [q for q in range(1, NSYM - 1) if starts[q] >= 0 and starts[q] + NSPS <= n_have]
    out["n_valid"] = len(valid)
    if len(valid) < RP_MIN_VALID:
        nan = float("nan")
        out.update(flags=RP_MEASURED | RP_INVALID, snr_db=nan, f_hz=nan, t_sec=nan, score=nan, on=nan, off=nan)
        if full:
            out["cells"] = np.zeros(0)
        return out
    C = report_symbols(G[it], delta)
    on = float(np.mean(np.abs(C[valid]) ** 2))
    fr = [fq + 8 * t for t in RP_CELLS if RP_FQ_LO <= fq + 8 * t <= RP_FQ_HI]
    off, cells = 0.0, np.zeros(0)
    if fr:
        hw = 0.5 - 0.5 * np.cos(2.0 * np.pi * (_N + 0.5) / NSPS)
        V = _symbols(x[:n_have], starts[valid]) * hw[None, :]
        H = V @ _phasors(fr).T
        cells = np.sort((H.real ** 2 + H.imag ** 2).reshape(-1))
        off = float(cells[(len(cells) - 1) // 4] / np.log(4.0 / 3.0) * NSPS / RP_HANN_SUM2)
    ratio = on / off - 1.0 if off > 0 else RP_SNR_FLOOR
    out.update(flags=flags, on=on, off=off, snr_db=float(10.0 * np.log10(max(ratio, RP_SNR_FLOOR) * TONE_HZ / 2500.0)),
               f_hz=fq * DF_HZ + delta * RP_DELTA_HZ, t_sec=(s0 + tau + 6.0 * dt) / FS)
    if full:
        out["cells"] = cells
    return out
