// ft4_report.hpp -- opt-in measured FT4 reports: SNR, frequency and start time of a decoded signal (extension; DESIGN.md section
// 19.9; ft8rx_ft4_report).  pyft8_amd/ft4.py holds the float64 twin that defines every step (report).  A decoded signal's 105 tones
// are known, so it is measured against its own model -- the subtraction's (ft4_sub.hpp: Ft4SubModel, ft4s_begin, ft4s_signal,
// ft4s_sample and the pulse table are used as they stand).  With y_tau[n] = x[s0 + tau + n] conj(s[n]), tau = -36, -30 .. 36, and
// x = 0 outside [0, n_have), everything is defined on the segment sums G_tau[j] = sum_{n < 36} y_tau[36 j + n], j < 1680:
//   k_ft4_rep_f32  the frames as float32, zero from n_have on: the select of the upper end is made once, here
//   k_ft4_rep_scan (pair of blocks of four symbols, row): a wavefront owns one block of four symbols, its lanes nine contiguous
//                  samples of a symbol each -- one evaluation of s[n] serves the 13 tau: 13 loads, 13 products.  A segment is the
//                  sum of four lanes; the block's G[13][64] lives in LDS only.  Then lane (tau, delta) forms
//                  C[q] = sum_{j < 16} G_tau[16 q + j] e^{-2 pi i delta (36 (16 q + j) + 17.5) / 12000}, delta = -6 .. 6 x 0.6510 Hz,
//                  and writes |sum_q C[q]|^2 -> part[row][block][169]
//   k_ft4_rep_pick (row; one wavefront): P = the 26 partials in block order; the first maximum in tau-major order; a three-point
//                  parabola on each axis where the peak is interior, else FT8RX_RP_EDGE_T / _F
//   k_ft4_rep_snr  (row): at the peak's tau and the interpolated delta, wavefront w takes every fourth valid symbol from the w-th on: the symbol
//                  sum C[q] again (`on` = the mean |C[q]|^2 of the valid symbols: 1 .. 103, wholly inside [0, n_have)) and the
//                  Hann-weighted cells of the same 576 samples at fq + 8 t, t = -5, -4, -3, 6, 7, 8 (a frequency outside [8, 2296]
//                  is dropped whole); `off` = the lower quartile of the cells by rank selection / ln(4/3) x 576 / 216.  Fewer than
//                  32 valid symbols: FT8RX_RP_INVALID and NaN fields
// Arithmetic: per-lane sums in fp32, cross-lane and cross-block sums in fp64 in a fixed order, no atomics: a report is the same bytes
// on every run, alone or in a batch.  Every phase is a fraction of a turn formed exactly in integers (the carrier's as in the
// subtraction; delta's is delta (72 j + 35) / 36864 of a turn; a cell's is (f n mod 4608) / 4608) -- the interpolated delta's in fp64.
#ifndef FT8RX_FT4_REPORT_HPP
#define FT8RX_FT4_REPORT_HPP

#define FT4R_NTAU 13                            /* trial starts -36, -30 .. +36 samples */
#define FT4R_TAU_STEP 6
#define FT4R_NDEL 13                            /* trial frequencies -6 .. +6 x 12000 / 18432 Hz */
#define FT4R_NP (FT4R_NTAU * FT4R_NDEL)         /* 169 */
#define FT4R_NBLK 26                            /* symbols 1 .. 103 in blocks of four: 25 whole ones and {101, 102, 103} */
#define FT4R_NCELL 6
#define FT4R_MAXCELLS ((FT4_NSYM - 2) * FT4R_NCELL)   /* 618 */
#define FT4R_MIN_VALID 32
#define FT4R_FQ_LO 8
#define FT4R_FQ_HI 2296
#define FT4R_SNR_FLOOR 1e-3f
#define FT4R_OFF_SCALE 9.2694941f               /* 576 / 216 / ln(4/3) */
static_assert(FT4R_NBLK * 4 >= FT4_NSYM - 2 && (FT4R_NBLK - 1) * 4 < FT4_NSYM - 2 && FT4R_NBLK % 2 == 0, "k_ft4_rep_scan: two blocks of four per thread block");

// what the pick hands to the SNR step
struct Ft4RepPeak { int32_t it, idl; float dt, dd, score; uint32_t flags; };

__global__ __launch_bounds__(256) void k_ft4_rep_f32(const int16_t* __restrict__ a, float* __restrict__ wf, int n_have) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < FT8RX_FT4_NSAMP) wf[(size_t)blockIdx.y * FT8RX_FT4_NSAMP + i] = i < n_have ? (float)a[(size_t)blockIdx.y * FT8RX_FT4_NSAMP + i] : 0.0f;
}

// the four lanes of a segment (lanes 4 g .. 4 g + 3) add up in fp64: (l0 + l1) + (l2 + l3) in every one of them
FT8_DEV void ft4r_seg_sum(double& vr, double& vi) {
    vr += __shfl_xor(vr, 1); vi += __shfl_xor(vi, 1);
    vr += __shfl_xor(vr, 2); vi += __shfl_xor(vi, 2);
}
// e^{-2 pi i d (72 j + 35) / 36864}: delta = d steps at the centre of segment j
FT8_DEV void ft4r_turn(int d, int j, float* c, float* s) {
    int ph = (d * (72 * j + 35)) % 36864;
    ph += ph < 0 ? 36864 : 0;
    const float fr = (float)ph * (1.0f / 36864.0f);
    *c = __builtin_amdgcn_cosf(fr); *s = -__builtin_amdgcn_sinf(fr);
}

// part [rows][FT4R_NBLK][FT4R_NP]
__global__ __launch_bounds__(128) void k_ft4_rep_scan(const float* __restrict__ wf, Ft4SubSel sel, const double* __restrict__ pc, float* __restrict__ part) {
    __shared__ Ft4SubModel M;
    __shared__ float2 G[2][FT4R_NTAU][64];
    const int row = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!ft4s_begin(sel, row, pc, &M)) return;
    const float* x = wf + (size_t)(sel.frame_of ? sel.frame_of[row] : row) * FT8RX_FT4_NSAMP;
    const int blk = 2 * blockIdx.x + wave;                    // < FT4R_NBLK
    const int q0 = 1 + 4 * blk, nq = blk == FT4R_NBLK - 1 ? 3 : 4;
    const int s0 = M.start - (FT4R_NTAU / 2) * FT4R_TAU_STEP;
#pragma unroll 1
    for (int qi = 0; qi < nq; qi++) {
        float ar[FT4R_NTAU], ai[FT4R_NTAU];
#pragma unroll
        for (int t = 0; t < FT4R_NTAU; t++) { ar[t] = 0.0f; ai[t] = 0.0f; }
#pragma unroll 1
        for (int j = 0; j < 9; j++) {
            const int r = 9 * lane + j;
            float sr, si;
            ft4s_signal(M, pc, q0 + qi, r, &sr, &si);
            const int g = s0 + FT4_NSPS * (q0 + qi) + r;
#pragma unroll
            for (int t = 0; t < FT4R_NTAU; t++) {
                const float xv = ft4s_sample(x, g + FT4R_TAU_STEP * t);
                ar[t] += xv * sr; ai[t] -= xv * si;           // y = x conj(s)
            }
        }
#pragma unroll
        for (int t = 0; t < FT4R_NTAU; t++) {
            double vr = (double)ar[t], vi = (double)ai[t];
            ft4r_seg_sum(vr, vi);
            if ((lane & 3) == 0) G[wave][t][16 * qi + (lane >> 2)] = make_float2((float)vr, (float)vi);
        }
    }
    __syncthreads();
    float* o = part + ((size_t)row * FT4R_NBLK + blk) * FT4R_NP;
#pragma unroll 1
    for (int p = lane; p < FT4R_NP; p += 64) {
        const int t = p / FT4R_NDEL, d = p - FT4R_NDEL * t - FT4R_NDEL / 2;
        double br = 0.0, bi = 0.0;
#pragma unroll 1
        for (int qi = 0; qi < nq; qi++) {
            float cr = 0.0f, ci = 0.0f;
#pragma unroll 4
            for (int j = 0; j < 16; j++) {
                const float2 g = G[wave][t][16 * qi + j];
                float c, s;
                ft4r_turn(d, 16 * (q0 + qi) + j, &c, &s);
                cr += g.x * c - g.y * s; ci += g.x * s + g.y * c;
            }
            br += (double)cr; bi += (double)ci;
        }
        o[p] = (float)(br * br + bi * bi);
    }
}

FT8_DEV bool ft4r_better(float v1, int i1, float v2, int i2) { return v1 > v2 || (v1 == v2 && i1 < i2); }
FT8_DEV float ft4r_parabola(float a, float b, float c) { const float den = a - 2.0f * b + c; return den != 0.0f ? 0.5f * (a - c) / den : 0.0f; }

// one wavefront per row.  scores [rows][FT4R_NP]: P, kept for the stage output
__global__ __launch_bounds__(64) void k_ft4_rep_pick(Ft4SubSel sel, const float* __restrict__ part, float* __restrict__ scores, Ft4RepPeak* __restrict__ peak) {
    __shared__ float P[FT4R_NP];
    const int row = blockIdx.x, lane = threadIdx.x;
    if (sel.s >= sel.counts[row]) return;
    float bv = -1.0f; int bi = 1 << 20;
    for (int p = lane; p < FT4R_NP; p += 64) {
        double v = 0.0;
        for (int b = 0; b < FT4R_NBLK; b++) v += (double)part[((size_t)row * FT4R_NBLK + b) * FT4R_NP + p];
        const float f = (float)v;
        P[p] = f; scores[(size_t)row * FT4R_NP + p] = f;
        if (ft4r_better(f, p, bv, bi)) { bv = f; bi = p; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o); const int oi = __shfl_xor(bi, o);
        if (ft4r_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    __syncthreads();
    if (lane == 0) {
        Ft4RepPeak k;
        k.it = bi / FT4R_NDEL; k.idl = bi - FT4R_NDEL * k.it; k.dt = 0.0f; k.dd = 0.0f; k.score = bv; k.flags = FT8RX_RP_MEASURED;
        if (k.it > 0 && k.it < FT4R_NTAU - 1) k.dt = ft4r_parabola(P[bi - FT4R_NDEL], bv, P[bi + FT4R_NDEL]); else k.flags |= FT8RX_RP_EDGE_T;
        if (k.idl > 0 && k.idl < FT4R_NDEL - 1) k.dd = ft4r_parabola(P[bi - 1], bv, P[bi + 1]); else k.flags |= FT8RX_RP_EDGE_F;
        peak[row] = k;
    }
}

// cell t of a signal at fq: t = 0 .. 5 -> 5, 4, 3 tones below tone 0 and 6, 7, 8 above (3, 4, 5 above tone 3)
FT8_DEV int ft4r_cell_fq(int fq, int t) { return fq + 8 * (t < 3 ? t - 5 : t + 3); }
FT8_DEV bool ft4r_cell_ok(int f) { return f >= FT4R_FQ_LO && f <= FT4R_FQ_HI; }

// rep [rows]; on_off [rows][2]
__global__ __launch_bounds__(256) void k_ft4_rep_snr(const float* __restrict__ wf, Ft4SubSel sel, const double* __restrict__ pc, const Ft4RepPeak* __restrict__ peak,
                                                     int n_have, ft8rx_report* __restrict__ rep, float* __restrict__ on_off) {
    __shared__ Ft4SubModel M;
    __shared__ float cell[FT4R_MAXCELLS], onv[FT4_NSYM], quart;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!ft4s_begin(sel, row, pc, &M)) return;
    const float* x = wf + (size_t)(sel.frame_of ? sel.frame_of[row] : row) * FT8RX_FT4_NSAMP;
    const Ft4RepPeak pk = peak[row];
    const int s0 = M.start + FT4R_TAU_STEP * (pk.it - FT4R_NTAU / 2);
    const double dsteps = (double)(pk.idl - FT4R_NDEL / 2) + (double)pk.dd;
    // the cell frequencies that stay, the same for every symbol: bit t of keep, nf of them
    unsigned keep = 0;
#pragma unroll
    for (int t = 0; t < FT4R_NCELL; t++) keep |= ft4r_cell_ok(ft4r_cell_fq(M.fq, t)) ? 1u << t : 0u;
    const int nf = __builtin_popcount(keep);
    // symbol q is valid where its 576 samples lie inside [0, n_have); the valid ones are a run q_lo .. q_hi
    int q_lo = 1, q_hi = FT4_NSYM - 2;
    if (s0 + FT4_NSPS * q_lo < 0) q_lo = (-s0 + FT4_NSPS - 1) / FT4_NSPS;
    if (s0 + FT4_NSPS * (q_hi + 1) > n_have) q_hi = (n_have - s0) / FT4_NSPS - 1;
    const int n_valid = q_hi >= q_lo ? q_hi - q_lo + 1 : 0;
    if (n_valid < FT4R_MIN_VALID) {                           // block-uniform
        if (tid == 0) {
            ft8rx_report o; memset(&o, 0, sizeof(o));
            o.snr_db = o.f_hz = o.t_sec = o.score = __builtin_nanf("");
            o.flags = FT8RX_RP_MEASURED | FT8RX_RP_INVALID;
            rep[row] = o;
            on_off[2 * (size_t)row] = on_off[2 * (size_t)row + 1] = __builtin_nanf("");
        }
        return;
    }
#pragma unroll 1
    for (int q = q_lo + wave; q <= q_hi; q += 4) {
        float ar = 0.0f, ai = 0.0f, hr[FT4R_NCELL], hi[FT4R_NCELL];
#pragma unroll
        for (int t = 0; t < FT4R_NCELL; t++) { hr[t] = 0.0f; hi[t] = 0.0f; }
#pragma unroll 1
        for (int j = 0; j < 9; j++) {
            const int r = 9 * lane + j;
            float sr, si;
            ft4s_signal(M, pc, q, r, &sr, &si);
            const float xv = ft4s_sample(x, s0 + FT4_NSPS * q + r);
            ar += xv * sr; ai -= xv * si;
            const float xw = xv * (0.5f - 0.5f * __builtin_amdgcn_cosf(((float)r + 0.5f) * (1.0f / (float)FT4_NSPS)));
#pragma unroll
            for (int t = 0; t < FT4R_NCELL; t++) {
                if ((keep >> t) & 1u) {
                    const float ph = (float)((ft4r_cell_fq(M.fq, t) * r) % 4608) * (1.0f / 4608.0f);
                    hr[t] += xw * __builtin_amdgcn_cosf(ph); hi[t] -= xw * __builtin_amdgcn_sinf(ph);
                }
            }
        }
        // the symbol sum: the segment's four lanes, its turn at the interpolated delta, the 16 segments
        double vr = (double)ar, vi = (double)ai;
        ft4r_seg_sum(vr, vi);
        {
            const int j = 16 * q + (lane >> 2);
            const double turns = dsteps * (double)(72 * j + 35) * (1.0 / 36864.0);
            const float f = (float)(turns - floor(turns));
            const double c = (double)__builtin_amdgcn_cosf(f), s = -(double)__builtin_amdgcn_sinf(f);
            const double tr = vr * c - vi * s, ti = vr * s + vi * c;
            vr = (lane & 3) == 0 ? tr : 0.0; vi = (lane & 3) == 0 ? ti : 0.0;
        }
        wave_sum2(vr, vi);
        if (lane == 0) onv[q] = (float)(vr * vr + vi * vi);
#pragma unroll
        for (int t = 0; t < FT4R_NCELL; t++) {
            if ((keep >> t) & 1u) {
                double cr = (double)hr[t], ci = (double)hi[t];
                wave_sum2(cr, ci);
                if (lane == 0) cell[(q - q_lo) * nf + __builtin_popcount(keep & ((1u << t) - 1u))] = (float)(cr * cr + ci * ci);
            }
        }
    }
    if (tid == 0) quart = 0.0f;
    __syncthreads();
    // rank selection of the lower quartile: ties by position, so the value found does not depend on the order of the list
    const int m = n_valid * nf;
    const int k = (m - 1) >> 2;
#pragma unroll 1
    for (int i = tid; i < m; i += 256) {
        const float v = cell[i];
        int rank = 0;
#pragma unroll 4
        for (int j = 0; j < m; j++) { const float u = cell[j]; rank += (u < v || (u == v && j < i)) ? 1 : 0; }
        if (rank == k) quart = v;
    }
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int q = q_lo; q <= q_hi; q++) acc += (double)onv[q];
        const float on = (float)(acc / (double)n_valid);
        const float off = m > 0 ? quart * FT4R_OFF_SCALE : 0.0f;
        const float ratio = off > 0.0f ? on / off - 1.0f : FT4R_SNR_FLOOR;
        ft8rx_report o; memset(&o, 0, sizeof(o));
        o.snr_db = 10.0f * log10f(fmaxf(ratio, FT4R_SNR_FLOOR) * (float)(20.0 + 5.0 / 6.0) * (1.0f / 2500.0f));
        o.f_hz = (float)((double)M.fq * (12000.0 / 4608.0) + dsteps * (12000.0 / 18432.0));
        o.t_sec = (float)(((double)s0 + (double)FT4R_TAU_STEP * (double)pk.dt) * (1.0 / 12000.0));
        o.score = pk.score;
        o.flags = pk.flags;
        rep[row] = o;
        on_off[2 * (size_t)row] = on; on_off[2 * (size_t)row + 1] = off;
    }
}

#endif
