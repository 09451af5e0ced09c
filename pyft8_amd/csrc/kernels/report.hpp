// report.hpp -- opt-in measured signal reports: SNR, frequency and start time of every decode (ft8rx_set_reports)
// Part of libft8rx.so; included by ft8rx.hip after fine_sync.hpp / recall.hpp.  Launched only for a batch enqueued with the setting on.
//
// A record's snr / tweaks are the reference's quantities: the spread of the payload grid and the search position.  Once a candidate
// has DECODED its 79 tones are known, and the signal can be measured with a matched correlation over all of them:
//   k_report_worklist (candidate)  lists the chunk's DECODED slots; every other slot's report is cleared
//   k_report          (item)       one 128-thread block per listed candidate, blocks stride over the list:
//       encode   word -> CRC-14 -> LDPC(174,91) (recall_encode) -> 79 tones (Costas blocks, Gray map)
//       series   z[0 .. 3199] of the slice at fb = 50 f0_idx + ftweak: ONE full fine_fft, held in LDS (unscaled and unconjugated:
//                every sum below is formed with conjugated twiddles, which leaves its modulus unchanged)
//       scan     P(tau, delta) = sum_s |sum_n z[tau + 32 s + n] e^{-2 pi i n (tone_s + delta) / 32}|^2 for tau = tb - 28 .. tb + 12 and
//                delta = -0.7 .. +0.7: thread (delta, group of ten symbols) forms the 32-sample sum once and slides it over the 41 tau
//                (one sample out, one in, one rotation), its 41 partial scores in registers; the eight groups add theirs in turn
//       peak     first maximum in tau-major order, a three-point parabola on each axis where the peak is interior
//       SNR      at the peak's integer tau and the interpolated delta: `on` = the mean rectangular |DFT|^2 at each symbol's own tone,
//                `off` = median / ln 2 * 32 / sum w^2 of the Hann-weighted cells more than two tones from the tones of the symbol and
//                of its neighbours; above on / off = RP_SWITCH without the cells of the two highest tones
// pyft8_amd/report.py is the float64 twin of every step.
#ifndef FT8RX_REPORT_HPP
#define FT8RX_REPORT_HPP

#define RP_NTAU 41
#define RP_TAU_LO (-28)
#define RP_NDEL 15
#define RP_SWITCH 300.0f
#define RP_TOP_TONE 6
#define RP_SNR_FLOOR 1e-3f
#define RP_OFF_SCALE 3.8471863f       /* 32 / sum w^2 / ln 2, sum w^2 = 12 for the half-sample Hann window */

// thread per candidate slot (256-thread blocks): DECODED slots go to the list, every other slot's report reads "none"
__global__ __launch_bounds__(256) void k_report_worklist(const ft8rx_record* __restrict__ rec, const int32_t* __restrict__ ncand, int B, int sh,
                                                         WorkList w, ft8rx_report* __restrict__ rep) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const bool in = c < (B << sh);
    const bool want = in && cand_live(c, B, sh, ncand) && rec[c].status == FT8RX_ST_DECODED;
    if (in && !want) { ft8rx_report z; memset(&z, 0, sizeof(z)); rep[c] = z; }
    work_push_block(w, want, c);
}

// sample i of the series, zero outside it (branch-free: a clamped load and a select)
FT8_DEV cpx rp_sample(const cpx* z, int i) {
    const bool ok = (unsigned)i < 3200u;
    const cpx v = z[ok ? i : 0];
    return make_float2(ok ? v.x : 0.0f, ok ? v.y : 0.0f);
}
// (value, index) order of the peak search: the larger value, ties to the smaller index
FT8_DEV bool rp_better(float v1, int i1, float v2, int i2) { return v1 > v2 || (v1 == v2 && i1 < i2); }
FT8_DEV float rp_parabola(float a, float b, float c) { const float den = a - 2.0f * b + c; return den != 0.0f ? 0.5f * (a - c) / den : 0.0f; }

// rank selection: the two middle values of list[0 .. m) -> med[0], med[1].  Every thread ranks its own entries against all (ties by
// position: the order of the list does not change the values found).
FT8_DEV void rp_median(const float* list, int m, float* med, int tid) {
    const int k0 = (m - 1) >> 1, k1 = m >> 1;
#pragma unroll 1
    for (int i = tid; i < m; i += FINE_NT) {
        const float v = list[i];
        int rank = 0;
#pragma unroll 4
        for (int j = 0; j < m; j++) { const float u = list[j]; rank += (u < v || (u == v && j < i)) ? 1 : 0; }
        if (rank == k0) med[0] = v;
        if (rank == k1) med[1] = v;
    }
}

static_assert(FINE_NT == 128, "k_report is written for 128 threads: 16 delta lanes x 8 symbol groups");
__global__ __launch_bounds__(FINE_NT, 2) void k_report(const cpx* __restrict__ spec, const ft8rx_record* __restrict__ rec,
                                                    ft8rx_report* __restrict__ rep, Tables T, int sh, WorkList work) {
    __shared__ cpx z[3200];
    __shared__ cpx w400[400];                 // the [4,4] stage's twiddles; dead after the transform, then the scores P[41][15]
    __shared__ cpx e320[320];                 // e^{+2 pi i j / 320}: every twiddle of the scan; then E[8][32] of the SNR step
    __shared__ float far_all[632], far_low[474];   // the far cells' powers, and those of the tones 0 .. RP_TOP_TONE - 1, in arrival order
    __shared__ float onv[80], hw[32], med[2], pk_v[2];
    __shared__ int pk_i[2], cnt[2];
    __shared__ uint64_t cwsh[3];
    __shared__ uint8_t tones[80];
    float* P = reinterpret_cast<float*>(w400);
    static_assert(sizeof(cpx) * 400 >= sizeof(float) * RP_NTAU * RP_NDEL, "P overlays w400");
    const int tid = threadIdx.x, lane = tid & 63;
    const int n_items = *work.count;
#pragma unroll 1
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int c = work.items[item];
        const int frame = c >> sh;
        const ft8rx_record r = rec[c];
        const int fb = 50 * (int)r.f0_idx + (int)r.ftweak;
        if (r.h0_idx < FT8RX_MIN_H0_FD || r.h0_idx > FT8RX_MAX_H0_FD || fb - 150 < 0 || fb + 850 > FT8RX_SPEC_BINS) {      // block-uniform
            if (tid == 0) {
                ft8rx_report o; memset(&o, 0, sizeof(o));
                o.snr_db = o.f_hz = o.t_sec = o.score = __builtin_nanf("");
                o.flags = FT8RX_RP_MEASURED | FT8RX_RP_INVALID;
                rep[c] = o;
            }
            continue;
        }
        // ---- tables and tones
        for (int i = tid; i < 400; i += FINE_NT) w400[i] = T.W3200[8 * i];
        for (int i = tid; i < 320; i += FINE_NT) { const cpx w = T.W3200[10 * i]; e320[i] = make_float2(w.x, -w.y); }
        if (tid < 32) hw[tid] = 0.5f - 0.5f * cospif(((float)tid + 0.5f) * 0.0625f);
        if (tid == 0) { uint64_t cw[3]; recall_encode(r.msg_lo, r.msg_hi, cw); cwsh[0] = cw[0]; cwsh[1] = cw[1]; cwsh[2] = cw[2]; }
        __syncthreads();
        if (tid < 79) {
            const int s = tid;
            int tone;
            if (s < 7) tone = d_COSTAS[s];
            else if (s >= 36 && s < 43) tone = d_COSTAS[s - 36];
            else if (s >= 72) tone = d_COSTAS[s - 72];
            else {
                const int v = 3 * (s < 36 ? s - 7 : s - 14);
                unsigned b = 0;
#pragma unroll
                for (int k = 0; k < 3; k++) b = (b << 1) | (unsigned)((cwsh[(v + k) >> 6] >> ((v + k) & 63)) & 1ull);
                tone = (int)((0x74652310u >> (4 * b)) & 7u);                          // Gray map 0 1 3 2 5 6 4 7
            }
            tones[s] = (uint8_t)tone;
        }
        // ---- the series (fine_fft ends with a barrier, which also publishes the tones)
        const cpx* __restrict__ Sg = spec + (size_t)frame * FT8RX_SPEC_BINS + (fb - 182);
        fine_fft(Sg, 182, z, w400, T, tid, 0, 3200);
        const int tb = 8 * (int)r.h0_idx + (r.h0_idx < 0 ? 1 : 0) + (int)r.ttweak;
        // ---- scan: thread (d, g) slides the symbols 10 g .. 10 g + 9 at delta = (d - 7) / 10
        const int d = tid & 15, g = tid >> 4;
        float acc[RP_NTAU];
#pragma unroll
        for (int i = 0; i < RP_NTAU; i++) acc[i] = 0.0f;
        if (d < RP_NDEL) {
            const int s_end = (10 * g + 10 < 79) ? 10 * g + 10 : 79;
#pragma unroll 1
            for (int s = 10 * g; s < s_end; s++) {
                int k = 10 * (int)tones[s] + d - 7;                                   // the symbol's frequency in 1/320 cycles per sample
                k += (k < 0) ? 320 : 0;
                const int base = tb + RP_TAU_LO + 32 * s;
                cpx S = make_float2(0.0f, 0.0f);
                int ph = 0;
#pragma unroll 8
                for (int n = 0; n < 32; n++) {
                    const cpx p = cmul(rp_sample(z, base + n), e320[ph]);
                    S.x += p.x; S.y += p.y;
                    ph += k; ph -= (ph >= 320) ? 320 : 0;
                }
                const cpx wout = e320[k ? 320 - k : 0];                               // e^{-i theta}
                const cpx win = e320[(31 * k) % 320];                                 // e^{+31 i theta}
                acc[0] += S.x * S.x + S.y * S.y;
#pragma unroll
                for (int i = 1; i < RP_NTAU; i++) {                                   // S(tau + 1) = (S(tau) - z[tau]) e^{-i theta} + z[tau + 32] e^{31 i theta}
                    const cpx a = rp_sample(z, base + i - 1), b = rp_sample(z, base + i + 31);
                    const cpx t1 = cmul(make_float2(S.x - a.x, S.y - a.y), wout), t2 = cmul(b, win);
                    S = make_float2(t1.x + t2.x, t1.y + t2.y);
                    acc[i] += S.x * S.x + S.y * S.y;
                }
            }
        }
        // the transform is done with w400: the eight groups add their partial scores in group order (the same sum in every run)
#pragma unroll 1
        for (int q = 0; q < 8; q++) {
            if (g == q && d < RP_NDEL) {
#pragma unroll
                for (int i = 0; i < RP_NTAU; i++) P[i * RP_NDEL + d] = (q ? P[i * RP_NDEL + d] : 0.0f) + acc[i];
            }
            __syncthreads();
        }
        // ---- peak: the first maximum in tau-major order
        {
            float bv = -1.0f; int bi = 1 << 20;
#pragma unroll 1
            for (int i = tid; i < RP_NTAU * RP_NDEL; i += FINE_NT) { const float v = P[i]; if (rp_better(v, i, bv, bi)) { bv = v; bi = i; } }
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o); const int oi = __shfl_xor(bi, o);
                if (rp_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if (lane == 0) { pk_v[tid >> 6] = bv; pk_i[tid >> 6] = bi; }
            if (tid < 2) cnt[tid] = 0;
            __syncthreads();
        }
        const bool first = rp_better(pk_v[0], pk_i[0], pk_v[1], pk_i[1]);
        const int pi = first ? pk_i[0] : pk_i[1];
        const float pv = first ? pk_v[0] : pk_v[1];
        const int it = pi / RP_NDEL, idl = pi - RP_NDEL * it;
        unsigned flags = FT8RX_RP_MEASURED;
        float dt = 0.0f, dd = 0.0f;
        if (it > 0 && it < RP_NTAU - 1) dt = rp_parabola(P[pi - RP_NDEL], pv, P[pi + RP_NDEL]); else flags |= FT8RX_RP_EDGE_T;
        if (idl > 0 && idl < RP_NDEL - 1) dd = rp_parabola(P[pi - 1], pv, P[pi + 1]); else flags |= FT8RX_RP_EDGE_F;
        const float delta = 0.1f * ((float)(idl - RP_NDEL / 2) + dd);
        const int tau = tb + RP_TAU_LO + it;
        __syncthreads();                                                              // every thread has read P and e320's scan twiddles
        // ---- SNR at (tau, delta): E[t][n] = e^{+2 pi i n (t + delta) / 32}
        cpx* E = e320;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int i = tid + FINE_NT * q, t = i >> 5, n = i & 31;
            float sn, cs;
            sincospif(((float)t + delta) * (float)n * 0.0625f, &sn, &cs);
            E[i] = make_float2(cs, sn);
        }
        __syncthreads();
#pragma unroll 1
        for (int q = 0; q < 5; q++) {
            const int i = tid + FINE_NT * q;
            if (i < 632) {
                const int s = i >> 3, t = i & 7;
                cpx R = make_float2(0.0f, 0.0f), H = make_float2(0.0f, 0.0f);
                const int base = tau + 32 * s;
#pragma unroll 8
                for (int n = 0; n < 32; n++) {
                    const cpx p = cmul(rp_sample(z, base + n), E[32 * t + n]);
                    R.x += p.x; R.y += p.y;
                    H.x = __builtin_fmaf(hw[n], p.x, H.x); H.y = __builtin_fmaf(hw[n], p.y, H.y);
                }
                const int t0 = tones[s], tm = tones[s > 0 ? s - 1 : s], tp = tones[s < 78 ? s + 1 : s];
                const bool far = abs(t - t0) > 2 && abs(t - tm) > 2 && abs(t - tp) > 2;
                if (t == t0) onv[s] = R.x * R.x + R.y * R.y;
                if (far) {
                    const float pw = H.x * H.x + H.y * H.y;
                    far_all[atomicAdd(&cnt[0], 1)] = pw;
                    if (t < RP_TOP_TONE) far_low[atomicAdd(&cnt[1], 1)] = pw;
                }
            }
        }
        __syncthreads();
        const int m_all = cnt[0], m_low = cnt[1];
        float on = 0.0f;
        for (int s = 0; s < 79; s++) on += onv[s];                                    // every thread: the same sum in the same order
        on *= (1.0f / 79.0f);
        float off = 0.0f;
        if (m_all > 0) {
            rp_median(far_all, m_all, med, tid);
            __syncthreads();
            off = 0.5f * (med[0] + med[1]) * RP_OFF_SCALE;
        }
        if (on > RP_SWITCH * off && m_low > 0) {                                      // block-uniform: the same on / off in every thread
            __syncthreads();                                                          // med has been read
            rp_median(far_low, m_low, med, tid);
            __syncthreads();
            off = 0.5f * (med[0] + med[1]) * RP_OFF_SCALE;
        }
        if (tid == 0) {
            const float ratio = off > 0.0f ? on / off - 1.0f : RP_SNR_FLOOR;
            ft8rx_report o; memset(&o, 0, sizeof(o));
            o.snr_db = 10.0f * log10f(fmaxf(ratio, RP_SNR_FLOOR) * 0.0025f);
            o.f_hz = 0.0625f * (float)fb + 6.25f * delta;
            o.t_sec = 0.005f * ((float)tau + dt);
            o.score = pv * (FINE_INV * FINE_INV);
            o.flags = flags;
            rep[c] = o;
        }
        __syncthreads();                                                              // the LDS images are reused by the next candidate
    }
}

#endif
