// recall.hpp -- ipass 8: recall decoding of stations heard 30 s earlier, by hypothesis (ft8rx_set_recall)
// Part of libft8rx.so; included by ft8rx.hip after fine_sync.hpp / llr.hpp.  Launched only for a batch that has recall entries set.
//
// A recall entry is a message the same stream decoded two cycles back (same parity) with its grid position.  Its station most likely
// sends a predictable continuation at the same place, so instead of searching for it the step tests a few known codewords there:
//   k_recall_stage  (frame)     the batch's entries -> the result slot's copy, the frame's recall records zeroed
//   k_recall_trip   (frame)     one (frame, f0_idx, h0_idx) triple per entry for k_fine / k_fine_td in trip mode (forced fine sync:
//                               the tweak scan runs, no sync threshold, no Costas gate, no llr_sd_min; the 79 x 8 grid is kept)
//   k_recall_score  (entry)     one wavefront: the skip rule, the LLRs of the grid (llr_from_p), up to 126 hypotheses (two per lane),
//                               CRC-14 + LDPC(174,91) encode, hard / soft distance, best and runner-up across the wave, the record
// Record e of a frame's recall area belongs to entry e.  An entry that does not qualify, or whose station a ladder record of the
// frame decoded (within +-2 f0 bins and +-4 h0 rows), writes nothing: its record stays zero (ipass 0).
#ifndef FT8RX_RECALL_HPP
#define FT8RX_RECALL_HPP

// LDPC(174,91) parity columns: d_RCG[j] = the 91 message bits (word 0: bits 0..63, word 1: bits 64..90) that parity bit 91 + j sums.
// The generator is systematic (codeword bits 0..90 = the message and its CRC), so a codeword costs 83 x 2 popcounts.
__device__ uint64_t d_RCG[83][2];

// entry kinds (ft8rx_recall_entry.pad, written by the host at ft8rx_set_recall): 0 = does not qualify, 1 = "A B X", 2 = "CQ B X"
enum { RC_SKIP = 0, RC_CALL = 1, RC_TOKEN = 2 };

__global__ void k_recall_stage(const ft8rx_recall_entry* __restrict__ src, const int32_t* __restrict__ src_cnt,
                               ft8rx_recall_entry* __restrict__ dst, int32_t* __restrict__ dst_cnt, ft8rx_record* __restrict__ rrec) {
    const int f = blockIdx.x, i = threadIdx.x;
    const int n = src_cnt[f];
    if (i < n) dst[(size_t)f * FT8RX_RECALL_MAX + i] = src[(size_t)f * FT8RX_RECALL_MAX + i];
    ft8rx_record z; memset(&z, 0, sizeof(z));
    rrec[(size_t)f * FT8RX_RECALL_MAX + i] = z;
    if (i == 0) dst_cnt[f] = n;
}

// triple of entry e of frame f at off[f] + e (off: the batch's per-frame prefix, frame-local indices as k_fine reads the spectrum)
__global__ void k_recall_trip(const ft8rx_recall_entry* __restrict__ ent, const int32_t* __restrict__ cnt, const int32_t* __restrict__ off,
                              int32_t* __restrict__ trip) {
    const int f = blockIdx.x, e = threadIdx.x;
    if (e >= cnt[f]) return;
    const ft8rx_recall_entry& E = ent[(size_t)f * FT8RX_RECALL_MAX + e];
    int32_t* t = trip + 3 * (size_t)(off[f] + e);
    t[0] = f; t[1] = E.f0_idx; t[2] = E.h0_idx;
}

// hypothesis k (0 .. 125) of an entry, in the order of ft8rx_recall_hypotheses: the entry's own word, then (A B only) RRR, RR73, 73,
// the reports -30 .. +30, the R-reports R-30 .. R+30.  The g15 field (bits 3..17) and the R flag (bit 18) are replaced; the calls,
// their /P or /R flags and i3 stay.  -> false for an index the entry does not have.
FT8_DEV bool recall_word(uint64_t lo, int kind, int k, uint64_t* out, int* cls) {
    if (k == 0) { *out = lo; *cls = 0; return true; }
    if (kind != RC_CALL || k >= 126) return false;
    unsigned g15, r = 0;
    if (k <= 3) { g15 = 32401u + (unsigned)k; *cls = k; }                   // 32402 RRR, 32403 RR73, 32404 73
    else if (k < 65) { g15 = (unsigned)(32435 + (k - 4) - 30); *cls = 4; }
    else { g15 = (unsigned)(32435 + (k - 65) - 30); r = 1; *cls = 5; }
    *out = (lo & ~(0xFFFFull << 3)) | ((uint64_t)g15 << 3) | ((uint64_t)r << 18);
    return true;
}

// 77-bit word (lo, hi) -> 174-bit codeword, codeword bit v at cw[v >> 6] bit v & 63 (the layout of hostmsg::encode_cw174)
FT8_DEV void recall_encode(uint64_t lo, uint64_t hi, uint64_t cw[3]) {
    hi &= 0x1FFFull;
    const unsigned crc = ft8_crc14(lo, hi);
    // bits 0..76 = word bits 76..0; bits 77..90 = CRC bits 13..0
    cw[0] = __builtin_bitreverse64((lo >> 13) | (hi << 51));
    cw[1] = (__builtin_bitreverse64(lo & 0x1FFFull) >> 51) | ((__builtin_bitreverse64((uint64_t)crc) >> 50) << 13);
    cw[2] = 0;
    const uint64_t m1 = cw[1];
#pragma unroll 1
    for (int j = 0; j < 83; j++) {
        const uint64_t b = (uint64_t)((__popcll(cw[0] & d_RCG[j][0]) + __popcll(m1 & d_RCG[j][1])) & 1);
        const int v = 91 + j;
        cw[v >> 6] |= b << (v & 63);
    }
}

// (D, index) order: smaller D first, ties in hypothesis order
FT8_DEV bool rc_less(float d1, int i1, float d2, int i2) { return d1 < d2 || (d1 == d2 && i1 < i2); }

// One wavefront per entry (block = 64).  t = base + blockIdx.x indexes the triple / its fine-sync outputs; offc[f] = the triple of the
// chunk's frame f's first entry; rec / ncand (nullable: ft8rx_recall_probe) the ladder's records of the chunk for the skip rule.
__global__ __launch_bounds__(64) void k_recall_score(const float* __restrict__ sgrid, const int32_t* __restrict__ tout,
                                                     const int32_t* __restrict__ trip, const int32_t* __restrict__ offc, int base,
                                                     const ft8rx_recall_entry* __restrict__ ent, const ft8rx_record* __restrict__ rec,
                                                     const int32_t* __restrict__ ncand, int sh, int max_hd, int min_gap,
                                                     ft8rx_record* __restrict__ rrec) {
    __shared__ float p[464], llr[176], sq[176];
    const int lane = threadIdx.x;
    const int t = base + blockIdx.x;
    const int f = trip[3 * (size_t)t], e = t - offc[f];
    const ft8rx_recall_entry E = ent[(size_t)f * FT8RX_RECALL_MAX + e];
    const int kind = E.pad;
    if (kind == RC_SKIP) return;                                              // block-uniform
    if (rec) {                                                                // the station was heard normally: nothing to recall
        const int n = ncand[f];
        bool hit = false;
        for (int c = lane; c < n; c += 64) {
            const ft8rx_record& r = rec[((size_t)f << sh) + c];
            hit |= r.status == FT8RX_ST_DECODED && abs((int)r.f0_idx - (int)E.f0_idx) <= 2 && abs((int)r.h0_idx - (int)E.h0_idx) <= 4;
        }
        if (__ballot(hit)) return;
    }
    const float* g = sgrid + (size_t)t * 632;
    for (int i = lane; i < 464; i += 64) p[i] = 20.0f * ft8_log10f(g[8 * (int)d_PAYSYM[i >> 3] + (i & 7)]);   // receiver.py:170
    __syncthreads();
    float sd; int snr;
    llr_from_p(p, llr, sq, lane, true, &sd, &snr);
    if (!(sd > 0.0f) || !isfinite(sd)) return;                                // a flat grid: no LLRs (sd is wave-uniform)
    const uint64_t h0 = __ballot(llr[lane] > 0.0f), h1 = __ballot(llr[64 + lane] > 0.0f), h2 = __ballot(lane < 46 && llr[128 + (lane < 46 ? lane : 0)] > 0.0f);
    const uint64_t lo = E.msg_lo, hi = E.msg_hi & 0x1FFFull;
    float D[2]; int hd[2], cls[2]; uint64_t w[2]; bool ok[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int k = lane + 64 * q;
        ok[q] = recall_word(lo, kind, k, &w[q], &cls[q]);
        if (ok[q] && k > 0 && w[q] == lo) ok[q] = false;                      // the repeat is hypothesis 0 already
        D[q] = __builtin_inff(); hd[q] = 175;
        if (!ok[q]) continue;
        uint64_t cw[3];
        recall_encode(w[q], hi, cw);
        uint64_t d0 = cw[0] ^ h0, d1 = cw[1] ^ h1, d2 = (cw[2] ^ h2) & ((1ull << 46) - 1);
        hd[q] = __popcll(d0) + __popcll(d1) + __popcll(d2);
        float s = 0.0f;
        while (d0) { s += fabsf(llr[__builtin_ctzll(d0)]); d0 &= d0 - 1; }
        while (d1) { s += fabsf(llr[64 + __builtin_ctzll(d1)]); d1 &= d1 - 1; }
        while (d2) { s += fabsf(llr[128 + __builtin_ctzll(d2)]); d2 &= d2 - 1; }
        D[q] = s;
    }
    // the list index after the dropped duplicate of the repeat (at most one: the hypotheses are distinct words)
    const int kd = [&] {
        uint64_t tmp; int c;
        const bool d_a = lane > 0 && recall_word(lo, kind, lane, &tmp, &c) && tmp == lo;
        const bool d_b = recall_word(lo, kind, lane + 64, &tmp, &c) && tmp == lo;
        const uint64_t ba = __ballot(d_a), bb = __ballot(d_b);
        return ba ? __builtin_ctzll(ba) : bb ? 64 + __builtin_ctzll(bb) : 1 << 20;
    }();
    int idx[2];
#pragma unroll
    for (int q = 0; q < 2; q++) { const int k = lane + 64 * q; idx[q] = ok[q] ? k - (k > kd ? 1 : 0) : (1 << 20) + k; }
    // best of the wave, then the best of the rest
    const int qb = rc_less(D[1], idx[1], D[0], idx[0]) ? 1 : 0;
    float bD = D[qb]; int bI = idx[qb], bH = hd[qb];
    for (int o = 32; o > 0; o >>= 1) {
        const float oD = __shfl_xor(bD, o); const int oI = __shfl_xor(bI, o), oH = __shfl_xor(bH, o);
        if (rc_less(oD, oI, bD, bI)) { bD = oD; bI = oI; bH = oH; }
    }
    const int q2 = (idx[0] == bI) ? 1 : (idx[1] == bI) ? 0 : qb;
    float sD = D[q2]; int sI = idx[q2], sH = hd[q2];
    for (int o = 32; o > 0; o >>= 1) {
        const float oD = __shfl_xor(sD, o); const int oI = __shfl_xor(sI, o), oH = __shfl_xor(sH, o);
        if (rc_less(oD, oI, sD, sI)) { sD = oD; sI = oI; sH = oH; }
    }
    const bool have2 = sI < (1 << 20);
    if (!have2) { sH = 174; }
    // the winner's word and class from the lane that holds it
    const int own = (idx[0] == bI) ? 0 : (idx[1] == bI) ? 1 : -1;
    const uint64_t wb = own >= 0 ? w[own] : 0ull;
    const int cb = own >= 0 ? cls[own] : 0;
    const uint64_t holder = __ballot(own >= 0);
    if (!holder) return;                                                      // no hypothesis at all (cannot happen: the repeat is valid)
    const int src = __builtin_ctzll(holder);
    const uint64_t word = ((uint64_t)__shfl((int)(uint32_t)(wb >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)wb, src);
    const int wcls = __shfl(cb, src);
    if (lane != 0) return;
    const bool accept = bH <= max_hd && sH - bH >= min_gap;              // no runner-up (a CQ's repeat alone): hd 174
    ft8rx_record r; memset(&r, 0, sizeof(r));
    r.msg_lo = word; r.msg_hi = hi;
    r.score = bD; r.grid_sd = have2 ? sD : -1.0f; r.fine_sd = sd;
    r.f0_idx = E.f0_idx; r.h0_idx = E.h0_idx;
    const int32_t* o = tout + 5 * (size_t)t;
    r.ttweak = (int8_t)o[1]; r.ftweak = (int8_t)o[2]; r.nsync = (uint8_t)o[3]; r.snr_fine = (int8_t)snr;
    r.status = accept ? FT8RX_ST_DECODED : FT8RX_ST_EXHAUSTED; r.ipass = 8; r.ap = (uint8_t)wcls; r.method = FT8RX_M_RECALL;
    r.n_its = (int16_t)bI; r.osd_hd = (uint8_t)bH; r.pad2 = (uint32_t)sH;
    rrec[(size_t)f * FT8RX_RECALL_MAX + e] = r;
}

#endif
