// ap_calls.hpp -- ipass 7: a-priori decoding with the operator's own and the DX station's callsigns (ft8rx_set_ap_calls)
// Part of libft8rx.so; included by ft8rx.hip after bp.hpp / osd.hpp.  Launched only while a call is set (enqueue_chain).
//
// After the reference's ladder (ipass 0..6) a candidate that is EXHAUSTED -- it passed the Costas gate and the sd check, so llr0 holds
// its fine LLRs, and no step decoded it -- gets one wavefront per enabled pattern (ap_patterns.hpp):
//   k_ap_worklist   (candidate)            the EXHAUSTED candidates
//   k_bp_ap         (candidate, pattern)   partial patterns: BP(nc0_b, iters_b) on the overridden LLRs (bp_attempt<.., AP7>); an
//                                          attempt whose BP found no valid word goes onto the OSD list (a valid word beyond the gate
//                                          ends the pattern); full patterns: the codeword's distance to the hard decisions
//   k_osd_ap        (candidate, pattern)   OSD of the same overridden LLRs (osd_attempt<.., AP7>); vectors with a NaN are skipped
//   k_select_ap     (candidate)            among the patterns that pass the gate, the smallest distance (ties: pattern order)
// Every attempt passes the gate "distance of the accepted codeword to the hard decisions of the UN-overridden fine LLRs <= max_hd";
// the distance goes to the record's osd_hd.  Attempt results reuse the OSD slots attO[candidate * 10 + pattern - 5] (dead once
// k_select2 has run).  Events: ipass 7, slot 2 * pattern for BP and the codeword test, 2 * pattern + 1 for OSD (the host replays
// them in that order), seq as in the ladder (BP iteration + 1, OSD trial, 0).
#ifndef FT8RX_AP_CALLS_HPP
#define FT8RX_AP_CALLS_HPP

// the setting, written on the chain's own stream (ft8rx.hip: enqueue_chain) into that chain's copy of the per-handle buffer: batches in
// flight keep what they started with, and no host memory has to outlive the call
__global__ void k_ap_stage(ApCalls* dst, ApCalls a) {
    if (threadIdx.x == 0) *dst = a;
}

// the ipass-7 work list: every candidate the reference's ladder left EXHAUSTED (thread per candidate)
__global__ void k_ap_worklist(const ft8rx_record* rec, const int32_t* ncand, int B, int sh, WorkList next) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = cand_live(c, B, sh, ncand) && rec[c].status == FT8RX_ST_EXHAUSTED;
    work_push_block(next, on, c);
}

// full pattern (8..10): the codeword is fixed, so BP / OSD could only ever return it -- count its disagreements with the hard decisions
FT8_DEV void ap_codeword_test(int lane, int c, int p, const float* __restrict__ llr0, Att* __restrict__ att7, ft8rx_event* ev,
                              int32_t* evcount, int sh, const ApCalls* __restrict__ a) {
    const float* src = llr0 + (size_t)c * 174;
    const int k = p - FT8RX_AP_FIRST;
    const uint64_t h0 = __ballot(src[lane] > 0.0f), h1 = __ballot(src[64 + lane] > 0.0f), h2 = __ballot(lane < 46 && src[128 + (lane < 46 ? lane : 0)] > 0.0f);
    const int hd = __popcll(h0 ^ a->val[k][0]) + __popcll(h1 ^ a->val[k][1]) + __popcll(h2 ^ a->val[k][2]);
    if (lane != 0) return;
    Att r; memset(&r, 0, sizeof(r)); r.n_its = 0;
    if (hd <= a->max_hd) {
        r.ok = 1; r.lo = a->lo[k]; r.hi = a->hi[k]; r.method = FT8RX_M_AP_CODEWORD; r.pad[0] = (uint8_t)hd;
        log_event(ev, evcount, c >> sh, c & ((1 << sh) - 1), 7, 2 * p, 0, r.lo, r.hi, 1);
    }
    att7[(size_t)c * 10 + k] = r;
}

// one wavefront per (candidate, pattern); a bounded grid strides over list x patterns (the host does not know the list's length)
__global__ __launch_bounds__(64, BP_WV) void k_bp_ap(const float* __restrict__ llr0, ft8rx_record* __restrict__ rec, const int32_t* __restrict__ ncand,
                                                     Att* __restrict__ att7, ft8rx_event* ev, int32_t* evcount, ft8rx_config cfg,
                                                     const ApCalls* __restrict__ apc, WorkList cands, WorkList osdl) {
    const int np = apc->np, n = *cands.count * np;
    _Pragma("unroll 1")
    for (int item = blockIdx.x; item < n; item += gridDim.x) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int c = cands.items[item / np], p = apc->pat[item % np];
        if (p >= 8) ap_codeword_test(tid, c, p, llr0, att7, ev, evcount, cand_shift(cfg), apc);
        else bp_attempt<false, true>(tid, 1, (c << 4) | p, llr0, rec, ncand, nullptr, att7, nullptr, ev, evcount, cfg,
                                     cfg.bp_nc0_b, cfg.bp_iters_b, 0u, apc, &osdl);
        __syncthreads();                                        // the LDS arrays are reused by the next attempt
    }
}

// OSD of the partial-pattern attempts BP left undecoded (list entries: candidate << 4 | pattern)
#define OSD_AP_KERNEL(NAME, WIDE)                                                                                                   \
__global__ __launch_bounds__(64) OSD_ATTR void NAME(const float* __restrict__ llr0, ft8rx_record* __restrict__ rec,                \
                                                    const int32_t* __restrict__ ncand, Att* __restrict__ att7, ft8rx_event* ev,     \
                                                    int32_t* evcount, const uint32_t* __restrict__ trials, int ntr, int nflip,      \
                                                    int sh, const ApCalls* __restrict__ apc, WorkList work) {                       \
    const OsdArgs a = {llr0, nullptr, nullptr, rec, ncand, att7, ev, evcount, trials, ntr, nflip, 0, sh, {nullptr, nullptr}, 0u, apc}; \
    osd_blocks<WIDE, false, false, true>(*work.count, 0, a, [&](int item) { return work.items[item]; });                            \
}
OSD_AP_KERNEL(k_osd_ap, false)
OSD_AP_KERNEL(k_osd_ap_wide, true)
#undef OSD_AP_KERNEL

// ipass 7's choice (thread per list entry): the accepted pattern with the smallest distance, ties in pattern order
__global__ void k_select_ap(ft8rx_record* rec, const Att* att7, const ApCalls* __restrict__ apc, WorkList cands) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *cands.count) return;
    const int c = cands.items[i], np = apc->np;
    int best = -1, bhd = 1 << 30;
    for (int k = 0; k < np; k++) {
        const int p = apc->pat[k];
        const Att& a = att7[(size_t)c * 10 + (p - FT8RX_AP_FIRST)];
        if (a.ok && (int)a.pad[0] < bhd) { best = p; bhd = a.pad[0]; }
    }
    if (best < 0) return;
    const Att& a = att7[(size_t)c * 10 + (best - FT8RX_AP_FIRST)];
    ft8rx_record& r = rec[c];
    r.status = FT8RX_ST_DECODED; r.ipass = 7; r.ap = (uint8_t)best; r.method = a.method; r.n_its = a.n_its;
    r.msg_lo = a.lo; r.msg_hi = a.hi; r.osd_hd = (uint8_t)bhd;
}

#endif
