// ft4_verify.hpp -- OSD on the coherent LLRs behind a whole-message score (opt-in, ft8rx_ft4_set_coh_osd).
// The run-of-2 and run-of-4 rows of k_ft4_coh go through OSD's raw-vector mode (k_osd*, untouched) under a wide distance gate; what
// decides is a coherent score of the decoded word against the audio.  The twin is pyft8_amd/ft4.py verify_score.
//   k_ft4_verify      one workgroup per OSD attempt: the word's 105 tones, the 105 x 4 complex sums of k_ft4_coh's steps 1 - 2 at the
//                     candidate's winner and q, then  score = A / sqrt(N),
//                       A = sum over the 26 runs R_k = {1 + 4 k .. min(4 + 4 k, 103)} of |sum_{s in R_k} C[s][T[s]]|,
//                       N = (1 / 412) sum_{s = 1 .. 103} sum_t |C[s][t]|^2;  0 where N = 0, near 206 on a clean signal
//   k_ft4_cosd_pos, k_ft4_cosd_gather, k_ft4_after_cosd: the step's bookkeeping (the coherent rows of OSD's list, the records and events)
// After ft4.hpp (the sample read, the phasor, the wave sum, the Costas tables) and recall.hpp (the device encoder and its parity rows).
#ifndef FT8RX_FT4_VERIFY_HPP
#define FT8RX_FT4_VERIFY_HPP

// Attempt i of n_att: list item li = i % n_list (the run-of-2 attempts of the n_list items, then the run-of-4 ones), candidate slot
// c = items[li] (items NULL: li), its row in k_ft4_coh's outputs p = pos[c] (pos NULL: li): q[p].  The word is att[i]'s (descrambled, as
// OSD's FT4 flag leaves it).  rec (nullable): the batch's records, for the early exit.  tones (nullable): [n_att][105].
__global__ __launch_bounds__(FT4_DEMOD_NT) void k_ft4_verify(const int16_t* __restrict__ audio, const int32_t* __restrict__ trip, const int32_t* __restrict__ tweak,
                                                             const int32_t* __restrict__ items, const int32_t* __restrict__ pos, const int32_t* __restrict__ q_in,
                                                             const Att* __restrict__ att, const ft8rx_record* __restrict__ rec, int n_list,
                                                             float* __restrict__ score, uint8_t* __restrict__ tones) {
    __shared__ cpx s_C[FT4_NSYM * 4];
    __shared__ cpx s_rot8[8], s_rot32[32];
    __shared__ uint64_t s_cw[3];
    __shared__ uint8_t s_T[FT4_NSYM + 3];
    __shared__ double s_run[FT4_COH_RUNS4], s_pw[FT4_NSYM];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = i % n_list;
    const int c = items ? items[li] : li;
    const Att a = att[i];
    if (!a.ok || (rec && rec[c].status == FT8RX_ST_DECODED)) {            // uniform per block, in front of the first barrier
        if (tid == 0) score[i] = 0.0f;
        return;
    }
    const int p = pos ? pos[c] : li;
    const int frame = trip[3 * c], f0 = trip[3 * c + 1], h0 = trip[3 * c + 2], tt = tweak[2 * c], ft = tweak[2 * c + 1], q = q_in[p];
    const int16_t* au = audio + (size_t)frame * FT8RX_FT4_NSAMP;
    const int fq0 = 4 * f0 + ft;
    if (tid < 32) { float sn, cs; sincospif(-(float)tid * (1.0f / 16.0f), &sn, &cs); s_rot32[tid] = make_float2(cs, sn); }
    else if (tid < 40) { float sn, cs; sincospif(-(float)(tid - 32) * 0.25f, &sn, &cs); s_rot8[tid - 32] = make_float2(cs, sn); }
    else if (tid == 64) {                                               // the word XOR rvec -> CRC-14 -> the 83 parity bits
        uint64_t cw[3];
        recall_encode(a.lo ^ FT4_RVEC_LO, a.hi ^ FT4_RVEC_HI, cw);
        s_cw[0] = cw[0]; s_cw[1] = cw[1]; s_cw[2] = cw[2];
    }
    __syncthreads();
    // ---- the tones: R S4a D29 S4b D29 S4c D29 S4d R, two codeword bits per data symbol through the Gray map 0 1 3 2
    if (tid < FT4_NSYM) {
        int t = 0;
        if (tid >= 1 && tid <= FT4_NSYM - 2) {
            if (ft4_is_sync(tid)) t = ft4_costas_at(tid);
            else {
                const int b0 = 2 * ft4_data_index(tid), b1 = b0 + 1;
                const int v = (int)((s_cw[b0 >> 6] >> (b0 & 63)) & 1ull) << 1 | (int)((s_cw[b1 >> 6] >> (b1 & 63)) & 1ull);
                t = v ^ (v >> 1);
            }
        }
        s_T[tid] = (uint8_t)t;
        if (tones) tones[(size_t)i * FT4_NSYM + tid] = (uint8_t)t;
    }
    // ---- k_ft4_coh's step 1: the 105 x 4 complex sums at the winner, each times tone 0's phase at the symbol's start -- and step 2's
    // turn by (q s mod 32) / 32, both from the exact tables
#pragma unroll 1
    for (int sym = wv; sym < FT4_NSYM; sym += FT4_DEMOD_NT / 64) {
        const int base = FT4_HOP * h0 + FT4_DT_STEP * tt + FT4_NSPS * sym;
        const cpx r8 = s_rot8[(fq0 * sym) & 7], r32 = s_rot32[(q * sym) & 31];
        float v[9];
#pragma unroll
        for (int j = 0; j < 9; j++) v[j] = ft4_sample(au, base + lane + 64 * j);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int fq = fq0 + 8 * t;
            float re = 0.0f, im = 0.0f;
#pragma unroll
            for (int j = 0; j < 9; j++) { const cpx w = ft4_phasor(fq, lane + 64 * j); re += v[j] * w.x; im -= v[j] * w.y; }
            re = ft4_wave_sum(re); im = ft4_wave_sum(im);
            if (lane == 0) {
                const cpx z = make_float2(re * r8.x - im * r8.y, re * r8.y + im * r8.x);
                s_C[4 * sym + t] = make_float2(z.x * r32.x - z.y * r32.y, z.x * r32.y + z.y * r32.x);
            }
        }
    }
    __syncthreads();
    // ---- A and N: fp64 sums of the fp32 amplitudes, every one in index order
    if (tid < FT4_COH_RUNS4) {
        double re = 0.0, im = 0.0;
        for (int s = 1 + 4 * tid; s <= 4 + 4 * tid && s <= FT4_NSYM - 2; s++) { const cpx z = s_C[4 * s + s_T[s]]; re += (double)z.x; im += (double)z.y; }
        s_run[tid] = sqrt(re * re + im * im);
    } else if (tid >= 64 && tid < 64 + FT4_NSYM) {
        const int s = tid - 64;
        double pw = 0.0;
        for (int t = 0; t < 4; t++) { const cpx z = s_C[4 * s + t]; pw += (double)z.x * (double)z.x + (double)z.y * (double)z.y; }
        s_pw[s] = pw;
    }
    __syncthreads();
    if (tid == 0) {
        double A = 0.0, N = 0.0;
        for (int k = 0; k < FT4_COH_RUNS4; k++) A += s_run[k];
        for (int s = 1; s <= FT4_NSYM - 2; s++) N += s_pw[s];
        N *= 1.0 / 412.0;
        score[i] = N > 0.0 ? (float)(A / sqrt(N)) : 0.0f;
    }
}

// pos[items[i]] = i: candidate slot -> its position in the first failure list, which indexes k_ft4_coh's rows
__global__ void k_ft4_cosd_pos(const int32_t* __restrict__ items, int n, int32_t* __restrict__ pos) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) pos[items[i]] = i;
}
// the run-of-2 rows, then the run-of-4 rows, of OSD's list, back to back: block i < 2 n copies row pos[items[i % n]] of half i / n
// (llr: the n_rows run-of-2 rows, then the n_rows run-of-4 rows)
__global__ __launch_bounds__(64) void k_ft4_cosd_gather(const float* __restrict__ llr, int n_rows, const int32_t* __restrict__ items, int n,
                                                        const int32_t* __restrict__ pos, float* __restrict__ dense) {
    const int i = blockIdx.x, half = i / n;
    const float* src = llr + ((size_t)half * n_rows + pos[items[i - half * n]]) * 174;
    float* dst = dense + (size_t)i * 174;
    for (int k = threadIdx.x; k < 174; k += 64) dst[k] = src[k];
}
// after OSD on the coherent rows (att / score [2 n]: the run-of-2 attempts of the n list items, then the run-of-4 ones) and
// k_ft4_verify: only a candidate left EXHAUSTED may become decoded, by a word whose score reaches min_score; run length 2 wins.  Such a
// decode is an OSD decode whose nsync carries the run length, whose pad2 carries rint(100 score) and whose event carries slot 1 or 2.
__global__ void k_ft4_after_cosd(ft8rx_record* __restrict__ rec, int sh, const Att* __restrict__ att, const float* __restrict__ score,
                                 const int32_t* __restrict__ items, int n, float min_score, ft8rx_event* ev, int32_t* evcount) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = items[i];
    ft8rx_record& r = rec[c];
    if (r.status != FT8RX_ST_EXHAUSTED) return;
    const Att a2 = att[i], a4 = att[n + i];
    const bool ok2 = a2.ok && score[i] >= min_score, ok4 = a4.ok && score[n + i] >= min_score;
    if (!ok2 && !ok4) return;
    const Att a = ok2 ? a2 : a4;
    const float sc = ok2 ? score[i] : score[n + i];
    r.status = FT8RX_ST_DECODED; r.ipass = 5; r.ap = 0; r.method = FT8RX_M_OSD; r.n_its = a.n_its; r.osd_hd = a.pad[0]; r.nsync = ok2 ? 2 : 4;
    r.pad2 = (uint32_t)rintf(100.0f * sc); r.msg_lo = a.lo; r.msg_hi = a.hi;
    log_event(ev, evcount, c >> sh, c & ((1 << sh) - 1), 5, ok2 ? 1 : 2, a.n_its, a.lo, a.hi, 1);
}

#endif
