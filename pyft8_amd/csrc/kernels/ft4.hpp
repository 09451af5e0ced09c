// ft4.hpp -- the FT4 front end (extension; ft8rx_ft4_*): spectrogram, four-block Costas search, fine sync and a
// symbol-synchronous demodulator for 7.5-s frames.  pyft8_amd/ft4.py holds the float64 twin that defines every stage; behind the
// LLRs the decoder is FT8's (k_bp_ext / k_osd_ext in raw-vector mode with the FT4 flag of ft8_dev.h: the 77 bits are descrambled
// between the CRC test and the validity predicate).
//   k_ft4_grid    P[r][k] = |rfft(hann_periodic(1152) x[144 r ..])|^2, r < 618, k < 577, as a 576-point complex FFT of the even / odd
//                 samples plus the real split; dB = 10 log10(max(P, 1e-24)) as the FT8 grid takes it
//   k_ft4_sync    per f0 the first strict maximum over h0 of the 16-symbol Costas score, fp64 sums of the fp32 dB values
//   k_ft4_peaks   threshold and neighbour suppression; k_topk (sync_search.hpp) then orders and cuts the survivors
//   k_ft4_demod   one workgroup per candidate: 9 x 5 fine trials on the 16 sync symbols, then the 105 x 4 amplitudes at the winner,
//                 LLRs, SNR.  A wave takes a symbol, its lanes split the 576 samples; the phasor of sample n at frequency
//                 fq x 12000 / 4608 Hz is (fq n mod 4608) / 4608 of a turn -- an exact integer phase, restarted per symbol
//   k_ft4_coh     opt-in (ft8rx_ft4_set_coherent), one workgroup per candidate BP left undecoded: the complex
//                 105 x 4 sums at the winner, a residual-frequency scan on the sync symbols, max-log LLRs over runs of 2 and 4 symbols
//   k_ft4_trip, k_ft4_after_bp, k_ft4_after_coh, k_ft4_gather, k_ft4_after_osd: the chain's bookkeeping (records, events, the OSD list)
// Samples outside [0, 90000) read as zero through a clamped address and a select: never an out-of-range load.
#ifndef FT8RX_FT4_HPP
#define FT8RX_FT4_HPP

#define FT4_NSPS 576
#define FT4_NSYM 105
#define FT4_HOP 144
#define FT4_NFFT 1152
#define FT4_GR 3                                 /* rows per workgroup of k_ft4_grid: 618 = 3 x 206 */
#define FT4_GRID_NT 128
#define FT4_GRID_SPAN (FT4_HOP * (FT4_GR - 1) + FT4_NFFT)      /* samples a workgroup reads, once: 1440 */
#define FT4_N_DT 9
#define FT4_N_DF 5
#define FT4_DT_STEP 36
#define FT4_DEMOD_NT 256
static_assert(FT8RX_FT4_ROWS % FT4_GR == 0 && FT4_HOP * (FT8RX_FT4_ROWS - 1) + FT4_NFFT == FT8RX_FT4_NSAMP &&
              FT8RX_FT4_COLS == FT4_NFFT / 2 + 1 && FT4_GRID_SPAN % 2 == 0 && (FT4_HOP * FT4_GR) % 2 == 0, "FT4 grid geometry");

// ------------------------------------------------------------------------------------ grid
// workgroup (g, f): rows 3 g .. 3 g + 2 of frame f.  win [1152] Hann (periodic), W576 [576] e^{-2 pi i t / 576}, WR [577] e^{-2 pi i k / 1152}.
// power (optional): the same layout as grid_db, the powers before the logarithm (the tests compare these with the twin's).
__global__ __launch_bounds__(FT4_GRID_NT) void k_ft4_grid(const int16_t* __restrict__ audio, float* __restrict__ grid_db, float* __restrict__ power,
                                                          const float* __restrict__ win, const cpx* __restrict__ W576, const cpx* __restrict__ WR) {
    __shared__ float xs[FT4_GRID_SPAN];
    __shared__ cpx za[FT4_GR * 576], zb[FT4_GR * 576];
    const int g = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    // the run's samples, once: 432 g + [0, 1440) lies inside the frame for every g < 206 (432 x 205 + 1440 = 90000); pairs are 4-byte aligned
    const uint32_t* a = reinterpret_cast<const uint32_t*>(audio + (size_t)f * FT8RX_FT4_NSAMP + (size_t)FT4_HOP * FT4_GR * g);
    for (int i = tid; i < FT4_GRID_SPAN / 2; i += FT4_GRID_NT) {
        const uint32_t raw = a[i];
        xs[2 * i] = (float)(int16_t)(raw & 0xFFFFu); xs[2 * i + 1] = (float)(int16_t)(raw >> 16);
    }
    __syncthreads();
    for (int i = tid; i < FT4_GR * 576; i += FT4_GRID_NT) {
        const int r = i / 576, m = i - r * 576;
        const float2 w = *reinterpret_cast<const float2*>(win + 2 * m);
        za[i] = make_float2(xs[FT4_HOP * r + 2 * m] * w.x, xs[FT4_HOP * r + 2 * m + 1] * w.y);
    }
    __syncthreads();
    const cpx* z = lds_fft<576, 8, 8, 3, 3>(za, zb, W576, FT4_GR, tid, FT4_GRID_NT);
    for (int i = tid; i < FT4_GR * FT8RX_FT4_COLS; i += FT4_GRID_NT) {
        const int r = i / FT8RX_FT4_COLS, k = i - r * FT8RX_FT4_COLS;
        const cpx p = z[r * 576 + (k == 576 ? 0 : k)], q2 = z[r * 576 + (k == 0 || k == 576 ? 0 : 576 - k)];
        const float er = 0.5f * (p.x + q2.x), ei = 0.5f * (p.y - q2.y);
        const float orr = 0.5f * (p.y + q2.y), oi = 0.5f * (q2.x - p.x);
        const cpx w = WR[k];
        const float xr = er + (w.x * orr - w.y * oi);
        const float xi = ei + (w.x * oi + w.y * orr);
        float pw = xr * xr + xi * xi;
        const size_t o = ((size_t)f * FT8RX_FT4_ROWS + (size_t)FT4_GR * g + r) * FT8RX_FT4_COLS + k;
        if (power) power[o] = pw;
        pw = (pw > 1e-24f) ? pw : 1e-24f;
        grid_db[o] = 10.0f * ft8_log10f_normal(pw);
    }
}

// ------------------------------------------------------------------------------------ search
// sync symbol ss = 4 b + s of Costas block b: symbol 1 + 33 b + s, tone (s ^ (s >> 1)) ^ b  (a = 0 1 3 2; b, c, d = a ^ 1, 2, 3)
FT8_DEV int ft4_sync_sym(int ss) { return 1 + 33 * (ss >> 2) + (ss & 3); }
FT8_DEV int ft4_sync_tone(int ss) { const int s = ss & 3; return (s ^ (s >> 1)) ^ (ss >> 2); }
// data symbol i < 87 -> its symbol index (three runs of 29 behind the sync blocks)
FT8_DEV int ft4_data_sym(int i) { return i < 29 ? 5 + i : i < 58 ? 9 + i : 13 + i; }

struct Ft4Range { int f0_lo, f0_hi, h0_lo, h0_hi; };      // f0_hi, h0_hi exclusive; 0 <= f0_lo < f0_hi <= 571 (tone 3 reads column f0 + 6)

// workgroup (t, f): f0 = f0_lo + 16 t + (tid & 15) of frame f, the h0 of the range over the 16 thread rows.  Rows outside the grid contribute 0.
__global__ __launch_bounds__(256) void k_ft4_sync(const float* __restrict__ grid, float* __restrict__ best_score, int32_t* __restrict__ best_h0, Ft4Range R) {
    __shared__ double redS[256];
    __shared__ int redH[256];
    const int f = blockIdx.y, tid = threadIdx.x, f0l = tid & 15;
    const int f0 = R.f0_lo + 16 * blockIdx.x + f0l;
    const bool on = f0 < R.f0_hi;
    const float* g = grid + (size_t)f * FT8RX_FT4_ROWS * FT8RX_FT4_COLS + (on ? f0 : R.f0_lo);
    double best = -INFINITY; int bh = R.h0_lo;
    for (int h0 = R.h0_lo + (tid >> 4); h0 < R.h0_hi; h0 += 16) {
        double sc = 0.0;
#pragma unroll 4
        for (int ss = 0; ss < 16; ss++) {
            const int row = h0 + 4 * ft4_sync_sym(ss) - 2, tone = ft4_sync_tone(ss);
            const bool in = row >= 0 && row < FT8RX_FT4_ROWS;
            const float* p = g + (size_t)(in ? row : 0) * FT8RX_FT4_COLS;
            const double d0 = (double)p[0], d1 = (double)p[2], d2 = (double)p[4], d3 = (double)p[6];
            const double own = tone == 0 ? d0 : tone == 1 ? d1 : tone == 2 ? d2 : d3;
            const double term = own + (-1.0 / 3.0) * ((((d0 + d1) + d2) + d3) - own);
            sc += in ? term : 0.0;
        }
        if (sc > best) { best = sc; bh = h0; }              // ascending h0: the first strict maximum of this thread row
    }
    redS[tid] = best; redH[tid] = bh;
    __syncthreads();
    if (tid < 16 && on) {
        double bs = redS[tid]; int h = redH[tid];
        for (int q = 1; q < 16; q++) {
            const double s = redS[tid + 16 * q]; const int hh = redH[tid + 16 * q];
            if (s > bs || (s == bs && hh < h)) { bs = s; h = hh; }
        }
        const size_t o = (size_t)f * NF0MAX + (f0 - R.f0_lo);
        best_score[o] = (float)bs; best_h0[o] = h;
    }
}

// kept[i] = raw[i] where raw[i] >= sync_min, raw[i - 1] < raw[i] and raw[i + 1] <= raw[i] (a tie goes to the lower bin), else 0: what
// k_topk (threshold 0) orders and cuts.  sync_min > 0 (ft8rx_ft4_set), so a kept score is positive.
__global__ void k_ft4_peaks(const float* __restrict__ raw, float* __restrict__ kept, int nf0, float sync_min, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (i >= nf0 || f >= B) return;
    const float* r = raw + (size_t)f * NF0MAX;
    const float s = r[i];
    const bool keep = s >= sync_min && !(i > 0 && r[i - 1] >= s) && !(i + 1 < nf0 && r[i + 1] > s);
    kept[(size_t)f * NF0MAX + i] = keep ? s : 0.0f;
}

// ------------------------------------------------------------------------------------ fine sync and demodulation
// the 576-sample DFT of frame samples base .. base + 575 at fq x 12000 / 4608 Hz, this lane's nine samples; reduce with ft4_wave_sum
FT8_DEV float ft4_sample(const int16_t* __restrict__ a, int idx) {
    const int ic = idx < 0 ? 0 : idx > FT8RX_FT4_NSAMP - 1 ? FT8RX_FT4_NSAMP - 1 : idx;
    const float v = (float)a[ic];
    return (idx >= 0 && idx < FT8RX_FT4_NSAMP) ? v : 0.0f;
}
FT8_DEV cpx ft4_phasor(int fq, int n) {
    const int ph = (fq * n) % 4608;                        // fq < 2400, n < 576: the product stays below 2^21
    float s, c;
    sincospif((float)ph * (1.0f / 2304.0f), &s, &c);
    return make_float2(c, s);
}
FT8_DEV float ft4_wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// trip [n][3] = (frame, f0, h0); frame < 0: an empty slot of the chain (zero LLRs, nothing else written).
// Outputs per candidate: llr [174], tweak [2] = (tt, ft), metric, snr.
__global__ __launch_bounds__(FT4_DEMOD_NT) void k_ft4_demod(const int16_t* __restrict__ audio, const int32_t* __restrict__ trip, float* __restrict__ llr,
                                                            int32_t* __restrict__ tweak, float* __restrict__ metric, int32_t* __restrict__ snr) {
    __shared__ float s_amp[FT4_N_DT * FT4_N_DF * 16];
    __shared__ float s_met[FT4_N_DT * FT4_N_DF];
    __shared__ float s_A[FT4_NSYM * 4];
    __shared__ float s_llr[176];
    __shared__ int s_best;
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int frame = trip[3 * c], f0 = trip[3 * c + 1], h0 = trip[3 * c + 2];
    float* out = llr + (size_t)c * 174;
    if (frame < 0) { if (tid < 174) out[tid] = 0.0f; return; }
    const int16_t* a = audio + (size_t)frame * FT8RX_FT4_NSAMP;
    // ---- the 45 trials on the 16 sync symbols
#pragma unroll 1
    for (int item = wv; item < FT4_N_DT * FT4_N_DF * 16; item += FT4_DEMOD_NT / 64) {
        const int trial = item >> 4, ss = item & 15;
        const int base = FT4_HOP * h0 + FT4_DT_STEP * (trial / FT4_N_DF - FT4_N_DT / 2) + FT4_NSPS * ft4_sync_sym(ss);
        const int fq = 4 * f0 + (trial % FT4_N_DF - FT4_N_DF / 2) + 8 * ft4_sync_tone(ss);
        float re = 0.0f, im = 0.0f;
#pragma unroll
        for (int j = 0; j < 9; j++) {
            const int n = lane + 64 * j;
            const float v = ft4_sample(a, base + n);
            const cpx w = ft4_phasor(fq, n);
            re += v * w.x; im -= v * w.y;
        }
        re = ft4_wave_sum(re); im = ft4_wave_sum(im);
        if (lane == 0) s_amp[item] = sqrtf(re * re + im * im);
    }
    __syncthreads();
    if (tid < FT4_N_DT * FT4_N_DF) {
        float m = 0.0f;
        for (int ss = 0; ss < 16; ss++) m += s_amp[16 * tid + ss];
        s_met[tid] = m;
    }
    __syncthreads();
    if (tid == 0) {
        int b = 0;
        for (int t = 1; t < FT4_N_DT * FT4_N_DF; t++) if (s_met[t] > s_met[b]) b = t;      // the first maximum in (dt, df) order
        s_best = b;
    }
    __syncthreads();
    const int best = s_best, tt = best / FT4_N_DF - FT4_N_DT / 2, ft = best % FT4_N_DF - FT4_N_DF / 2;
    // ---- the 105 x 4 amplitudes at the winner
#pragma unroll 1
    for (int sym = wv; sym < FT4_NSYM; sym += FT4_DEMOD_NT / 64) {
        const int base = FT4_HOP * h0 + FT4_DT_STEP * tt + FT4_NSPS * sym;
        float v[9];
#pragma unroll
        for (int j = 0; j < 9; j++) v[j] = ft4_sample(a, base + lane + 64 * j);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int fq = 4 * f0 + ft + 8 * t;
            float re = 0.0f, im = 0.0f;
#pragma unroll
            for (int j = 0; j < 9; j++) { const cpx w = ft4_phasor(fq, lane + 64 * j); re += v[j] * w.x; im -= v[j] * w.y; }
            re = ft4_wave_sum(re); im = ft4_wave_sum(im);
            if (lane == 0) s_A[4 * sym + t] = sqrtf(re * re + im * im);
        }
    }
    __syncthreads();
    // ---- max-log LLRs on amplitudes through the inverse Gray map: tones 2, 3 carry MSB = 1, tones 1, 2 carry LSB = 1
    if (tid < 87) {
        const float* A = s_A + 4 * ft4_data_sym(tid);
        s_llr[2 * tid] = fmaxf(A[2], A[3]) - fmaxf(A[0], A[1]);
        s_llr[2 * tid + 1] = fmaxf(A[1], A[2]) - fmaxf(A[0], A[3]);
    }
    __syncthreads();
    if (wv == 0) {                                         // scale 2.83 / std (population), all zeros where std = 0
        float s = 0.0f;
        for (int i = lane; i < 174; i += 64) s += s_llr[i];
        const float mean = ft4_wave_sum(s) / 174.0f;
        float q = 0.0f;
        for (int i = lane; i < 174; i += 64) { const float d = s_llr[i] - mean; q += d * d; }
        const float sd = sqrtf(ft4_wave_sum(q) / 174.0f);
        // an LLR of exactly 0 (a symbol outside the frame) becomes +0.001: k_bp's message update divides by tanh(llr / 2)
        for (int i = lane; i < 174; i += 64) { const float v = sd > 0.0f ? (2.83f * s_llr[i]) / sd : 0.0f; out[i] = (sd > 0.0f && v == 0.0f) ? 1e-3f : v; }
    } else if (wv == 1) {                                  // SNR from the matrix's powers
        float S = 0.0f, N = 0.0f;
        for (int sym = lane; sym < FT4_NSYM; sym += 64) {
            const float p0 = s_A[4 * sym] * s_A[4 * sym], p1 = s_A[4 * sym + 1] * s_A[4 * sym + 1], p2 = s_A[4 * sym + 2] * s_A[4 * sym + 2],
                        p3 = s_A[4 * sym + 3] * s_A[4 * sym + 3];
            const float top = fmaxf(fmaxf(p0, p1), fmaxf(p2, p3));
            S += top; N += ((((p0 + p1) + p2) + p3) - top) / 3.0f;
        }
        S = ft4_wave_sum(S) / (float)FT4_NSYM; N = ft4_wave_sum(N) / (float)FT4_NSYM;
        if (lane == 0) {
            int r = -24;
            if (N > 0.0f && S > N) {
                const float d = rintf(10.0f * log10f((S - N) / N) - 20.79181246f);      // 10 log10(2500 / 20.8333)
                r = d < -24.0f ? -24 : d > 24.0f ? 24 : (int)d;
            }
            snr[c] = r; tweak[2 * c] = tt; tweak[2 * c + 1] = ft; metric[c] = s_met[best];
        }
    }
}

// ------------------------------------------------------------------------------------ coherent LLRs (opt-in, ft8rx_ft4_set_coherent)
// DESIGN.md section 19.8; the twin is ft4.coherent_llrs.  One workgroup per item of a dense list (items NULL: item i is slot i); slot
// c = items[i] names the candidate trip[3 c ..] and its fine-sync winner tweak[2 c ..].  Outputs per item: q, metrics [9], llr2 and
// llr4 [174] each.
//   1  C[s][t] = the demodulator's 576-sample sums at the winner, kept complex, times e^{-2 pi i (fq s mod 8) / 8}: tone 0's phase
//      advances fq / 8 of a turn per symbol, an exact eighth; rot8 and rot32 below are the two tables
//   2  M(q), q = -4 .. 4: per Costas block |sum of its four C[s][costas] e^{-2 pi i (q s mod 32) / 32}|, the blocks added in order; the
//      first maximum; then row s of C turns by (q s mod 32) / 32
//   3  runs of 2 and of 4 symbols from symbol 1 on.  A lane is one assignment: two bits per symbol of the run, a sync symbol takes
//      its Costas tone whatever its two bits say and a symbol past 103 adds nothing, so the surplus lanes repeat assignments -- harmless
//      under max.  Per bit max{a : bit = 1} - max{a : bit = 0}: a butterfly over the other lane bits leaves each half's maximum in
//      the half's lanes.  Runs of 2: 16 lanes, finished in the wave.  Runs of 4: the 256 threads, the four waves' halves meet in LDS
//      once, behind the loop over the runs.  max is order-free: nothing depends on scheduling.
//   4  each row scaled like the demodulator's
#define FT4_COH_NQ 9
#define FT4_COH_RUNS4 26                         /* ceil(103 / 4); the last one (101 .. 103) is all sync */
#define FT4_COH_RUNS2 52                         /* ceil(103 / 2); the last one (103) is sync */
FT8_DEV bool ft4_is_sync(int s) { return (s - 1) % 33 < 4; }                       // s = 1 .. 103
FT8_DEV int ft4_costas_at(int s) { const int k = (s - 1) % 33; return (k ^ (k >> 1)) ^ ((s - 1) / 33); }
FT8_DEV int ft4_data_index(int s) { return s - 5 - 4 * ((s - 1) / 33); }            // inverse of ft4_data_sym
// symbol s of a run under the 2-bit value v of its lane
FT8_DEV cpx ft4_coh_term(const cpx* C, int s, int v) {
    if (s > FT4_NSYM - 2) return make_float2(0.0f, 0.0f);
    return C[4 * s + (ft4_is_sync(s) ? ft4_costas_at(s) : (v ^ (v >> 1)))];
}
// max over the lanes that agree with this lane in bit j of the lane id, among the NB low bits
template <int NB> FT8_DEV float ft4_half_max(float a, int j) {
    float v = a;
#pragma unroll
    for (int b = 0; b < NB; b++) { const float o = __shfl_xor(v, 1 << b); v = (b == j) ? v : fmaxf(v, o); }
    return v;
}
// the 174 raw differences in s_raw -> out: 2.83 / std (population), all zeros where std = 0, an exact 0 becomes +0.001 (one wave)
FT8_DEV void ft4_scale_llrs(const float* s_raw, float* __restrict__ out, int lane) {
    float s = 0.0f;
    for (int i = lane; i < 174; i += 64) s += s_raw[i];
    const float mean = ft4_wave_sum(s) / 174.0f;
    float q = 0.0f;
    for (int i = lane; i < 174; i += 64) { const float d = s_raw[i] - mean; q += d * d; }
    const float sd = sqrtf(ft4_wave_sum(q) / 174.0f);
    for (int i = lane; i < 174; i += 64) { const float v = sd > 0.0f ? (2.83f * s_raw[i]) / sd : 0.0f; out[i] = (sd > 0.0f && v == 0.0f) ? 1e-3f : v; }
}

__global__ __launch_bounds__(FT4_DEMOD_NT) void k_ft4_coh(const int16_t* __restrict__ audio, const int32_t* __restrict__ trip, const int32_t* __restrict__ tweak,
                                                          const int32_t* __restrict__ items, int32_t* __restrict__ q_out, float* __restrict__ metrics,
                                                          float* __restrict__ llr2, float* __restrict__ llr4) {
    __shared__ cpx s_C[FT4_NSYM * 4];
    __shared__ cpx s_rot8[8], s_rot32[32];
    __shared__ float s_blk[FT4_COH_NQ * 4], s_met[FT4_COH_NQ];
    __shared__ float s_half[FT4_COH_RUNS4][4][14];           // per run and wave: bits 0 .. 5 x (bit = 0, bit = 1), [12] the wave's maximum
    __shared__ float s_l2[176], s_l4[176];
    __shared__ int s_q;
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c = items ? items[i] : i;
    const int frame = trip[3 * c], f0 = trip[3 * c + 1], h0 = trip[3 * c + 2], tt = tweak[2 * c], ft = tweak[2 * c + 1];
    const int16_t* a = audio + (size_t)frame * FT8RX_FT4_NSAMP;
    const int fq0 = 4 * f0 + ft;
    if (tid < 32) { float sn, cs; sincospif(-(float)tid * (1.0f / 16.0f), &sn, &cs); s_rot32[tid] = make_float2(cs, sn); }
    else if (tid < 40) { float sn, cs; sincospif(-(float)(tid - 32) * 0.25f, &sn, &cs); s_rot8[tid - 32] = make_float2(cs, sn); }
    __syncthreads();
    // ---- 1: the 105 x 4 complex sums at the winner (k_ft4_demod's loop), each times tone 0's phase at the symbol's start
#pragma unroll 1
    for (int sym = wv; sym < FT4_NSYM; sym += FT4_DEMOD_NT / 64) {
        const int base = FT4_HOP * h0 + FT4_DT_STEP * tt + FT4_NSPS * sym;
        const cpx r = s_rot8[(fq0 * sym) & 7];
        float v[9];
#pragma unroll
        for (int j = 0; j < 9; j++) v[j] = ft4_sample(a, base + lane + 64 * j);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int fq = fq0 + 8 * t;
            float re = 0.0f, im = 0.0f;
#pragma unroll
            for (int j = 0; j < 9; j++) { const cpx w = ft4_phasor(fq, lane + 64 * j); re += v[j] * w.x; im -= v[j] * w.y; }
            re = ft4_wave_sum(re); im = ft4_wave_sum(im);
            if (lane == 0) s_C[4 * sym + t] = make_float2(re * r.x - im * r.y, re * r.y + im * r.x);
        }
    }
    __syncthreads();
    // ---- 2: the nine metrics, the first maximum, the rotation per symbol
    if (tid < FT4_COH_NQ * 4) {
        const int qi = tid >> 2, b = tid & 3;
        float re = 0.0f, im = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int s = 1 + 33 * b + k;
            const cpx z = s_C[4 * s + ft4_sync_tone(4 * b + k)], r = s_rot32[((qi - 4) * s) & 31];
            re += z.x * r.x - z.y * r.y; im += z.x * r.y + z.y * r.x;
        }
        s_blk[tid] = sqrtf(re * re + im * im);
    }
    __syncthreads();
    if (tid < FT4_COH_NQ) s_met[tid] = ((s_blk[4 * tid] + s_blk[4 * tid + 1]) + s_blk[4 * tid + 2]) + s_blk[4 * tid + 3];
    __syncthreads();
    if (tid == 0) {
        int b = 0;
        for (int t = 1; t < FT4_COH_NQ; t++) if (s_met[t] > s_met[b]) b = t;
        s_q = b - 4; q_out[i] = b - 4;
    }
    if (tid < FT4_COH_NQ) metrics[(size_t)i * FT4_COH_NQ + tid] = s_met[tid];
    __syncthreads();
    const int q = s_q;
    for (int e = tid; e < FT4_NSYM * 4; e += FT4_DEMOD_NT) {
        const cpx z = s_C[e], r = s_rot32[(q * (e >> 2)) & 31];
        s_C[e] = make_float2(z.x * r.x - z.y * r.y, z.x * r.y + z.y * r.x);
    }
    __syncthreads();
    // ---- 3a: runs of 2 -- 16 lanes per run, 16 runs per sweep of the block
    for (int run = tid >> 4; run < FT4_COH_RUNS2; run += FT4_DEMOD_NT / 16) {
        const int s0 = 1 + 2 * run;
        const cpx z0 = ft4_coh_term(s_C, s0, tid & 3), z1 = ft4_coh_term(s_C, s0 + 1, (tid >> 2) & 3);
        const float re = z0.x + z1.x, im = z0.y + z1.y;
        const float amp = sqrtf(re * re + im * im);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float mine = ft4_half_max<4>(amp, j), other = __shfl_xor(mine, 1 << j);
            const int s = s0 + (j >> 1);
            if ((tid & 15) == 0 && s <= FT4_NSYM - 2 && !ft4_is_sync(s)) s_l2[2 * ft4_data_index(s) + 1 - (j & 1)] = other - mine;      // lane bits all 0: mine = the bit-0 half
        }
    }
    // ---- 3b: runs of 4 -- the block is the 256 assignments; lane bits 0 .. 5 are symbols 0 .. 2 of the run, the wave is symbol 3
#pragma unroll 1
    for (int run = 0; run < FT4_COH_RUNS4; run++) {
        const int s0 = 1 + 4 * run;
        const cpx z0 = ft4_coh_term(s_C, s0, lane & 3), z1 = ft4_coh_term(s_C, s0 + 1, (lane >> 2) & 3), z2 = ft4_coh_term(s_C, s0 + 2, (lane >> 4) & 3),
                  z3 = ft4_coh_term(s_C, s0 + 3, wv);
        const float re = ((z0.x + z1.x) + z2.x) + z3.x, im = ((z0.y + z1.y) + z2.y) + z3.y;
        const float amp = sqrtf(re * re + im * im);
        float* hm = s_half[run][wv];
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const float mine = ft4_half_max<6>(amp, j);
            if (lane == 0) hm[2 * j] = mine;
            if (lane == (1 << j)) hm[2 * j + 1] = mine;
            if (j == 0) { const float all = fmaxf(mine, __shfl_xor(mine, 1)); if (lane == 0) hm[12] = all; }
        }
    }
    __syncthreads();
    if (tid < FT4_COH_RUNS4 * 8) {                           // the one LDS combine: thread = (run, bit j of the 8-bit assignment)
        const int run = tid >> 3, j = tid & 7, s = 1 + 4 * run + (j >> 1);
        float m0, m1;
        if (j < 6) {
            m0 = fmaxf(fmaxf(s_half[run][0][2 * j], s_half[run][1][2 * j]), fmaxf(s_half[run][2][2 * j], s_half[run][3][2 * j]));
            m1 = fmaxf(fmaxf(s_half[run][0][2 * j + 1], s_half[run][1][2 * j + 1]), fmaxf(s_half[run][2][2 * j + 1], s_half[run][3][2 * j + 1]));
        } else {                                             // symbol 3's value is the wave: bit 6 = waves 1, 3, bit 7 = waves 2, 3
            const float w0 = s_half[run][0][12], w1 = s_half[run][1][12], w2 = s_half[run][2][12], w3 = s_half[run][3][12];
            m0 = j == 6 ? fmaxf(w0, w2) : fmaxf(w0, w1);
            m1 = j == 6 ? fmaxf(w1, w3) : fmaxf(w2, w3);
        }
        if (s <= FT4_NSYM - 2 && !ft4_is_sync(s)) s_l4[2 * ft4_data_index(s) + 1 - (j & 1)] = m1 - m0;
    }
    __syncthreads();
    // ---- 4: the two rows, scaled
    if (wv == 0) ft4_scale_llrs(s_l2, llr2 + (size_t)i * 174, lane);
    else if (wv == 1) ft4_scale_llrs(s_l4, llr4 + (size_t)i * 174, lane);
}

// ------------------------------------------------------------------------------------ the chain's bookkeeping
// slot c of the batch -> its triple, frame -1 for a slot k_topk left empty
__global__ void k_ft4_trip(const ft8rx_record* __restrict__ rec, const int32_t* __restrict__ ncand, int B, int sh, int32_t* __restrict__ trip) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (B << sh)) return;
    const bool live = cand_live(c, B, sh, ncand);
    trip[3 * c] = live ? (c >> sh) : -1; trip[3 * c + 1] = live ? rec[c].f0_idx : 0; trip[3 * c + 2] = live ? rec[c].h0_idx : 0;
}

// after BP (k_bp_ext, raw vectors, att[c]): the demodulator's results into the records; a decoded slot gets its word (descrambled by
// the CRC check) and one event, an undecoded live one goes onto the OSD list.  256-thread blocks (work_push_block).
__global__ __launch_bounds__(256) void k_ft4_after_bp(ft8rx_record* __restrict__ rec, const int32_t* __restrict__ ncand, int B, int sh, const Att* __restrict__ att,
                                                      const int32_t* __restrict__ tweak, const int32_t* __restrict__ snr, ft8rx_event* ev, int32_t* evcount,
                                                      WorkList osdl) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    bool want = false;
    if (cand_live(c, B, sh, ncand)) {
        ft8rx_record& r = rec[c];
        r.grid_sd = r.score; r.fine_sd = r.score;            // the message layer replays in score order
        r.ttweak = (int8_t)tweak[2 * c]; r.ftweak = (int8_t)tweak[2 * c + 1]; r.snr_fine = (int8_t)snr[c]; r.snr_grid = (int8_t)snr[c];
        const Att a = att[c];
        if (a.ok) {
            r.status = FT8RX_ST_DECODED; r.ipass = 4; r.ap = 0; r.method = FT8RX_M_LDPC_B; r.n_its = a.n_its; r.msg_lo = a.lo; r.msg_hi = a.hi;
            log_event(ev, evcount, c >> sh, c & ((1 << sh) - 1), 4, 0, a.n_its + 1, a.lo, a.hi, 1);
        } else want = true;
    }
    work_push_block(osdl, want, c);
}
// after the coherent BPs (opt-in; att [2 n]: the run-of-2 attempts of the n list items, then the run-of-4 ones): run length 2 wins; a
// decode is a BP decode whose nsync carries the run length and whose event carries slot 1 or 2; the rest goes onto OSD's list
__global__ __launch_bounds__(256) void k_ft4_after_coh(ft8rx_record* __restrict__ rec, int sh, const Att* __restrict__ att, const int32_t* __restrict__ items,
                                                       int n, ft8rx_event* ev, int32_t* evcount, WorkList osdl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool want = false; int c = 0;
    if (i < n) {
        c = items[i];
        const Att a2 = att[i], a4 = att[n + i];
        if (a2.ok || a4.ok) {
            const Att a = a2.ok ? a2 : a4;
            ft8rx_record& r = rec[c];
            r.status = FT8RX_ST_DECODED; r.ipass = 4; r.ap = 0; r.method = FT8RX_M_LDPC_B; r.n_its = a.n_its; r.nsync = a2.ok ? 2 : 4;
            r.msg_lo = a.lo; r.msg_hi = a.hi;
            log_event(ev, evcount, c >> sh, c & ((1 << sh) - 1), 4, a2.ok ? 1 : 2, a.n_its + 1, a.lo, a.hi, 1);
        } else want = true;
    }
    work_push_block(osdl, want, c);
}
// the LLR rows of the OSD list, back to back: block i copies row items[i]
__global__ __launch_bounds__(64) void k_ft4_gather(const float* __restrict__ llr, const int32_t* __restrict__ items, float* __restrict__ dense) {
    const float* src = llr + (size_t)items[blockIdx.x] * 174;
    float* dst = dense + (size_t)blockIdx.x * 174;
    for (int i = threadIdx.x; i < 174; i += 64) dst[i] = src[i];
}
// after OSD (raw vectors, attO[i] of list item i): decoded or exhausted
__global__ void k_ft4_after_osd(ft8rx_record* __restrict__ rec, int sh, const Att* __restrict__ attO, const int32_t* __restrict__ items, int n,
                                ft8rx_event* ev, int32_t* evcount) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = items[i];
    ft8rx_record& r = rec[c];
    const Att a = attO[i];
    if (a.ok) {
        r.status = FT8RX_ST_DECODED; r.ipass = 5; r.ap = 0; r.method = FT8RX_M_OSD; r.n_its = a.n_its; r.osd_hd = a.pad[0]; r.msg_lo = a.lo; r.msg_hi = a.hi;
        log_event(ev, evcount, c >> sh, c & ((1 << sh) - 1), 5, 0, a.n_its, a.lo, a.hi, 1);
    } else r.status = FT8RX_ST_EXHAUSTED;
}

#endif
