// ft4_weak.hpp -- the FT4 weak search (opt-in, ft8rx_ft4_set_weak): coherent Costas sync on the 2.6042-Hz
// grid.  It stands in for k_ft4_grid and k_ft4_sync and fills the same per-f0 arrays, so k_ft4_peaks and k_topk follow unchanged.
// pyft8_amd/ft4.py holds the float64 twin (weak_grid, weak_score_map, search_weak) that defines both kernels.
//   k_ft4_cgrid   G[r][fq'] = sum_{n < 576} x[144 r + n] e^{-2 pi i (fq' (144 r + n) mod 4608) / 4608}, r = -3 .. 624 (every row with a
//                 sample inside the frame), fq' = 0 .. 2305.  Tone t of carrier fq is G[r][fq + 8 t] times i^(t r): one grid serves the
//                 four tones.  fq' = 8 m + j: the row's samples times e^{-2 pi i j n / 4608}, a 576-point transform, bin m.  The samples
//                 are real, so the transform of mix j holds mix -j too: conj(Z_j[576 - m']) is carrier 8 m' - j.  Five transforms per row
//                 (j = 0 .. 4) instead of eight; then a turn by (fq' r mod 32) / 32 for the row's start
//   k_ft4_csync   score(fq, h) = (|B_0| + .. + |B_3|) / sqrt(N) over fq = 4 f0 - 2 .. 4 f0 + 1 and the h0 range; per f0 the first
//                 maximum in (fq, h) order.  fp64 sums of the fp32 grid in a fixed order: nothing depends on scheduling
// Samples outside [0, 90000) and rows outside -3 .. 624 read as zero through a clamped address and a select: never an out-of-range load.
#ifndef FT8RX_FT4_WEAK_HPP
#define FT8RX_FT4_WEAK_HPP

#define FT4W_NFQ 2306                            /* carriers of the grid: f0 = 570 reads 4 f0 + 1 + 24 = 2305 */
#define FT4W_ROW_LO (-3)
#define FT4W_ROWS 628                            /* rows -3 .. 624 */
#define FT4W_NMIX 5
#define FT4W_CR 4                                /* rows per workgroup of k_ft4_cgrid: 628 = 4 x 157 */
#define FT4W_NT 256
#define FT4W_SPAN (FT4_HOP * (FT4W_CR - 1) + FT4_NSPS)          /* samples a workgroup reads, once: 1008 */
static_assert(FT4_HOP * FT4W_ROW_LO + FT4_NSPS > 0 && FT4_HOP * (FT4W_ROW_LO - 1) + FT4_NSPS <= 0 &&
              FT4_HOP * (FT4W_ROW_LO + FT4W_ROWS - 1) < FT8RX_FT4_NSAMP && FT4_HOP * (FT4W_ROW_LO + FT4W_ROWS) >= FT8RX_FT4_NSAMP &&
              4 * (FT8RX_FT4_COLS - 7) + 1 + 24 == FT4W_NFQ - 1 && FT4W_ROWS % FT4W_CR == 0, "FT4 weak grid geometry");

// ------------------------------------------------------------------------------------ complex grid
// workgroup (g, f): rows row_lo + 4 g .. + 3 of frame f, those below row_hi; -3 <= row_lo, row_hi <= 625 (the host clips).
// mix [5][576] e^{-2 pi i j n / 4608}, rot [32] e^{-2 pi i k / 32}, W576 [576] e^{-2 pi i t / 576}; G [frames][628][2306].
__global__ __launch_bounds__(FT4W_NT) void k_ft4_cgrid(const int16_t* __restrict__ audio, cpx* __restrict__ G, const cpx* __restrict__ mix,
                                                       const cpx* __restrict__ rot, const cpx* __restrict__ W576, int row_lo, int row_hi) {
    __shared__ float xs[FT4W_SPAN];
    __shared__ cpx za[FT4W_NMIX * 576], zb[FT4W_NMIX * 576];
    const int f = blockIdx.y, tid = threadIdx.x, r0 = row_lo + FT4W_CR * blockIdx.x;
    const int16_t* a = audio + (size_t)f * FT8RX_FT4_NSAMP;
    for (int i = tid; i < FT4W_SPAN; i += FT4W_NT) xs[i] = ft4_sample(a, FT4_HOP * r0 + i);
    __syncthreads();
#pragma unroll 1
    for (int rr = 0; rr < FT4W_CR; rr++) {
        const int r = r0 + rr;
        if (r >= row_hi) break;                                // uniform over the workgroup
        for (int i = tid; i < FT4W_NMIX * 576; i += FT4W_NT) {
            const int n = i % 576;
            const float v = xs[FT4_HOP * rr + n];
            const cpx w = mix[i];
            za[i] = make_float2(v * w.x, v * w.y);
        }
        __syncthreads();
        // radix order 3 3 8 8: 960 butterflies per radix-3 pass fill the 256 threads, and no pass is one of k_ft4_grid's plan (8 8 3 3),
        // whose code and registers stay as they are
        const cpx* z = lds_fft<576, 3, 3, 8, 8>(za, zb, W576, FT4W_NMIX, tid, FT4W_NT);
        cpx* out = G + ((size_t)f * FT4W_ROWS + (size_t)(r - FT4W_ROW_LO)) * FT4W_NFQ;
        for (int q = tid; q < FT4W_NFQ; q += FT4W_NT) {
            const int res = q & 7, m0 = q >> 3;
            const bool up = res > 4;                           // carrier 8 (m0 + 1) - (8 - res): the upper half of mix 8 - res, conjugated
            cpx v = z[(up ? 8 - res : res) * 576 + (up ? 575 - m0 : m0)];
            v.y = up ? -v.y : v.y;
            out[q] = cmul(v, rot[(q * r) & 31]);
        }
        __syncthreads();                                       // the transform's result lies in za or zb: the next row refills za
    }
}

// ------------------------------------------------------------------------------------ score
// i^q times v
FT8_DEV void ft4w_turn(cpx v, int q, double& re, double& im) {
    const float x = (q & 1) ? ((q & 2) ? v.y : -v.y) : ((q & 2) ? -v.x : v.x);
    const float y = (q & 1) ? ((q & 2) ? -v.x : v.x) : ((q & 2) ? -v.y : v.y);
    re += (double)x; im += (double)y;
}
// workgroup (t, f): the 16 f0 bins f0_lo + 16 t .. of frame f; lane = (f0, fq = 4 f0 - 2 + (lane & 3)), the four waves split the h0 of the
// range.  Per (fq, h) the 16 sync symbols in order, their four tones in order.  Writes what k_ft4_sync writes.
__global__ __launch_bounds__(256) void k_ft4_csync(const cpx* __restrict__ G, float* __restrict__ best_score, int32_t* __restrict__ best_h0, Ft4Range R) {
    __shared__ double redS[256];
    __shared__ int redH[256];
    const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int f0 = R.f0_lo + 16 * blockIdx.x + (lane >> 2), fq = 4 * f0 - 2 + (lane & 3);
    const bool on = f0 < R.f0_hi && fq >= 0;
    const int fqc = fq < 0 ? 0 : fq > FT4W_NFQ - 25 ? FT4W_NFQ - 25 : fq;
    const cpx* g = G + (size_t)f * FT4W_ROWS * FT4W_NFQ + fqc;
    double best = on ? -1.0 : -2.0; int bh = R.h0_lo;
#pragma unroll 1
    for (int h = R.h0_lo + wv; h < R.h0_hi; h += 4) {
        double E = 0.0, S = 0.0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            double re = 0.0, im = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int r = h + 4 * (1 + 33 * b + k), tone = ft4_sync_tone(4 * b + k);
                const bool in = r >= FT4W_ROW_LO && r < FT4W_ROW_LO + FT4W_ROWS;
                const cpx* p = g + (size_t)((in ? r : FT4W_ROW_LO) - FT4W_ROW_LO) * FT4W_NFQ;
                cpx v[4];
#pragma unroll
                for (int t = 0; t < 4; t++) { const cpx w = p[8 * t]; v[t] = make_float2(in ? w.x : 0.0f, in ? w.y : 0.0f); }
#pragma unroll
                for (int t = 0; t < 4; t++) E += (double)v[t].x * (double)v[t].x + (double)v[t].y * (double)v[t].y;
                ft4w_turn(v[tone], tone * h, re, im);          // i^(tone r): r = h mod 4
            }
            S += sqrt(re * re + im * im);
        }
        const double sc = E > 0.0 ? 8.0 * S / sqrt(E) : 0.0;
        if (sc > best) { best = sc; bh = h; }                  // ascending h: the first maximum of this wave's rows
    }
    redS[tid] = best; redH[tid] = bh;
    __syncthreads();
    if (tid < 16 && R.f0_lo + 16 * (int)blockIdx.x + tid < R.f0_hi) {
        double bs = -3.0; int h = R.h0_lo;
        for (int q = 0; q < 4; q++) {                          // fq ascending: a later fq wins only when strictly higher
            double s = redS[4 * tid + q]; int hh = redH[4 * tid + q];
            for (int w = 1; w < 4; w++) {
                const double s2 = redS[64 * w + 4 * tid + q]; const int h2 = redH[64 * w + 4 * tid + q];
                if (s2 > s || (s2 == s && h2 < hh)) { s = s2; hh = h2; }
            }
            if (s > bs) { bs = s; h = hh; }
        }
        const size_t o = (size_t)f * NF0MAX + (16 * blockIdx.x + tid);
        best_score[o] = (float)bs; best_h0[o] = h;
    }
}

#endif
