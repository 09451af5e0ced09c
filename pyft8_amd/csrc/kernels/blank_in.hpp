// Input-rate noise blanker (extension; ft8rx_blank_in*): impulse blanking of one stream of raw integer samples
// at its own rate, in front of whichever down-converter the rate takes, in integers, so that pyft8_amd/blank_in.py: reference() gives
// the same bits.  Section 17's blanker with three differences: the samples are real or IQ, 16 or 8 bits; the block is a power of two B
// in 256 .. 4096 anchored to the ABSOLUTE sample index; nothing is clamped -- outside the stream a = 0.
//   c     = x (int16), s (int8), 2 u - 255 (uint8);  a[n] = |c| (real) or |cI| + |cQ| (IQ), at most 65536
//   m_b   = element B / 2 of the sorted a of block b                                                   k_blankin_level
//   L_b   = element 2 of the sorted m[b - 2 .. b + 2] (m = 0 outside the stream)
//   hit   = L_b > 0 and 256 a[n] > threshold_q8 L_b                                                    k_blankin_hits
//   w[n]  = 0 within `guard` samples of a hit, the raised-cosine table T over the next `taper`, 32768 beyond;
//   c'    = (c w[n] + 16384) >> 15 per component, stored as int16 / int8 c' or uint8 (c' + 255) >> 1   k_blankin_gate
// The kernels see a WINDOW of the stream: x points at the sample of absolute index `base` (a multiple of B), samples outside [v0, v1)
// are outside the stream or not there yet and are never read; a launch covers a range of blocks (level, hits) or of samples (gate)
// that csrc/blank_in_ring.hpp works out per push.  Levels and the hit mask live in rings indexed by the absolute block / byte, so a
// push finds what the pushes before it left: m of the two blocks before, the hits within guard + taper before its first sample.
// As in section 17 k_blankin_hits derives every hit before k_blankin_gate rewrites a sample, a thread owns 8 consecutive samples =
// one byte of the mask, and the gate rewrites only its own samples inside [g0, g1): in place is safe, and a sample beyond g1 keeps
// its raw value for the push that releases it.
// Statistics: per-block partials that every block writes in full, summed into the stream's int64 counters by k_blankin_stats: exact,
// no atomics.
// VEC = x is 16-byte aligned: a group that lies wholly inside the stream goes by 16-byte accesses; the groups at the stream's ends,
// and every group of a buffer that is only component-aligned, go sample by sample.
// FMT: the format (sample_fmt.hpp; SF_REAL_I16, SF_IQ_I16, SF_IQ_U8 or SF_IQ_I8), a compile-time parameter; NC, CB, SB below are its
// components per sample, bytes per component and bytes per sample.
#pragma once

#define BIN_NT 256
#define BIN_HALO 128                   // guard + taper at most
#define BIN_TAPER_ROW 65               // the taper table of section 17: row R holds T[1 .. R] at [R][1 .. R]

// the window of a launch: x = the sample of absolute index base; [v0, v1) = the samples that exist
struct BinWin { char* x; long long base, v0, v1; };

// component values of the 8 samples from absolute index n0 (a multiple of 8) on; samples outside [v0, v1) give 0 and are not read
template <int FMT, bool VEC> FT8_DEV void bin_load8(const BinWin& W, long long n0, int c[8 * sf_components(FMT)]) {
    constexpr int NC = sf_components(FMT), CB = sf_component_bytes(FMT), SB = sf_sample_bytes(FMT);
    const char* p = W.x + (n0 - W.base) * SB;
    if (VEC && n0 >= W.v0 && n0 + 8 <= W.v1) {
#pragma unroll
        for (int q = 0; q < SB / 2; q++) {
            const int4 v = reinterpret_cast<const int4*>(p)[q];
            const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if constexpr (CB == 2) {
                    c[8 * q + 2 * i] = (int16_t)(w[i] & 0xffff); c[8 * q + 2 * i + 1] = w[i] >> 16;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int u = (w[i] >> (8 * k)) & 0xff;
                        c[4 * i + k] = FMT == SF_IQ_U8 ? 2 * u - 255 : (int)(int8_t)u;
                    }
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const bool in = n0 + j >= W.v0 && n0 + j < W.v1;
#pragma unroll
            for (int k = 0; k < NC; k++) {
                int v = 0;
                if (in) {
                    if (CB == 2) v = reinterpret_cast<const int16_t*>(p)[NC * j + k];
                    else if (FMT == SF_IQ_U8) v = 2 * (int)reinterpret_cast<const uint8_t*>(p)[NC * j + k] - 255;
                    else v = reinterpret_cast<const int8_t*>(p)[NC * j + k];
                }
                c[NC * j + k] = v;
            }
        }
    }
}
// ... and back: the samples of the group inside [g0, g1), nothing else
template <int FMT, bool VEC> FT8_DEV void bin_store8(const BinWin& W, long long n0, long long g0, long long g1, const int c[8 * sf_components(FMT)]) {
    constexpr int NC = sf_components(FMT), CB = sf_component_bytes(FMT), SB = sf_sample_bytes(FMT);
    char* p = W.x + (n0 - W.base) * SB;
    if (VEC && n0 >= g0 && n0 + 8 <= g1) {
#pragma unroll
        for (int q = 0; q < SB / 2; q++) {
            int w[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if constexpr (CB == 2) {
                    w[i] = (int)(((uint32_t)c[8 * q + 2 * i] & 0xffffu) | ((uint32_t)c[8 * q + 2 * i + 1] << 16));
                } else {
                    uint32_t u = 0;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int v = c[4 * i + k];
                        u |= ((uint32_t)(FMT == SF_IQ_U8 ? (v + 255) >> 1 : v) & 0xffu) << (8 * k);
                    }
                    w[i] = (int)u;
                }
            }
            reinterpret_cast<int4*>(p)[q] = make_int4(w[0], w[1], w[2], w[3]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (n0 + j < g0 || n0 + j >= g1) continue;
#pragma unroll
            for (int k = 0; k < NC; k++) {
                const int v = c[NC * j + k];
                if (CB == 2) reinterpret_cast<int16_t*>(p)[NC * j + k] = (int16_t)v;
                else if (FMT == SF_IQ_U8) reinterpret_cast<uint8_t*>(p)[NC * j + k] = (uint8_t)((v + 255) >> 1);
                else reinterpret_cast<int8_t*>(p)[NC * j + k] = (int8_t)v;
            }
        }
    }
}
template <int FMT> FT8_DEV void bin_mag8(const int c[8 * sf_components(FMT)], int a[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (sf_components(FMT) == 1) a[j] = c[j] < 0 ? -c[j] : c[j];
        else a[j] = (c[2 * j] < 0 ? -c[2 * j] : c[2 * j]) + (c[2 * j + 1] < 0 ? -c[2 * j + 1] : c[2 * j + 1]);
    }
}
FT8_DEV int bin_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
// the block's sums of a and b -> pa[0], pa[1].  Every thread of the block calls it (it holds a barrier); thread 0 stores.
FT8_DEV void bin_block_sums(int a, int b, int32_t* __restrict__ pa) {
    __shared__ int s_a[BIN_NT / 64], s_b[BIN_NT / 64];
    a = bin_wave_sum(a); b = bin_wave_sum(b);
    if ((threadIdx.x & 63) == 0) { s_a[threadIdx.x >> 6] = a; s_b[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) { pa[0] = s_a[0] + s_a[1] + s_a[2] + s_a[3]; pa[1] = s_b[0] + s_b[1] + s_b[2] + s_b[3]; }
}
FT8_DEV void bin_sort2(int& a, int& b) { const int lo = a < b ? a : b, hi = a < b ? b : a; a = lo; b = hi; }

// m_b by exact selection: one workgroup per block lv0 + blockIdx.x, thread t holds the groups t and t + 256 of the block's B / 8 (none
// beyond them: B <= 4096).  a <= 65536 < 2^17, so 17 steps from bit 16 down build the largest r with #{a < r} <= B / 2 = the element
// at sorted position B / 2.  A step's count: the thread's own, summed over the wave by shuffles and over the four waves through LDS
// (two buffers in turn: one barrier per step).  lv: the level ring [lv_cap][2], m at [0]; lv_cap a power of two.
template <int FMT, bool VEC>
__global__ __launch_bounds__(BIN_NT) void k_blankin_level(BinWin W, int log2_b, long long lv0, int32_t* __restrict__ lv, int lv_cap) {
    __shared__ int s_cnt[2][BIN_NT / 64];
    const long long b = lv0 + blockIdx.x;
    const int n_groups = 1 << (log2_b - 3), tid = threadIdx.x;
    int a[2][8];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int g = tid + q * BIN_NT;
        if (g < n_groups) {
            int c[8 * sf_components(FMT)];
            bin_load8<FMT, VEC>(W, (b << log2_b) + 8 * g, c);
            bin_mag8<FMT>(c, a[q]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) a[q][j] = 0x7fffffff;
        }
    }
    const int half = 1 << (log2_b - 1);
    int r = 0;
#pragma unroll 1
    for (int bit = 16; bit >= 0; bit--) {
        const int c = r | (1 << bit);
        int below = 0;
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
            for (int j = 0; j < 8; j++) below += a[q][j] < c ? 1 : 0;
        below = bin_wave_sum(below);
        if ((tid & 63) == 0) s_cnt[bit & 1][tid >> 6] = below;
        __syncthreads();
        below = s_cnt[bit & 1][0] + s_cnt[bit & 1][1] + s_cnt[bit & 1][2] + s_cnt[bit & 1][3];
        if (below <= half) r = c;
    }
    if (tid == 0) lv[2 * (size_t)(b & (lv_cap - 1))] = r;
}

// Hit flags of the blocks hb0 .. hb1 - 1, their L_b, and the workgroup's share of the counters `hits` (part[..][0]) and `complete blocks
// with L_b = 0` (part[..][1]).  Thread t of the launch owns the samples hb0 B + 8 t .. + 7 and their byte of the mask ring (mask_cap
// bytes, a power of two; absolute byte n / 8), which it always writes.  m exists for the blocks [b_first, b_have) and is 0 elsewhere;
// a block counts as complete below cb_end.
template <int FMT, bool VEC>
__global__ __launch_bounds__(BIN_NT) void k_blankin_hits(BinWin W, int log2_b, long long hb0, long long hb1, long long b_first, long long b_have,
                                                         long long cb_end, int32_t threshold_q8, int32_t* __restrict__ lv, int lv_cap,
                                                         uint8_t* __restrict__ mask, long long mask_cap, int32_t* __restrict__ part) {
    const long long t = (long long)blockIdx.x * BIN_NT + threadIdx.x, n0 = (hb0 << log2_b) + 8 * t, b = n0 >> log2_b;
    const bool live = b < hb1;
    int L = 0;
    bool leader = false;
    if (live) {
        int m[5];
#pragma unroll
        for (int d = 0; d < 5; d++) { const long long q = b + d - 2; m[d] = q >= b_first && q < b_have ? lv[2 * (size_t)(q & (lv_cap - 1))] : 0; }
        // element 2 of five: after these exchanges m[2] is the median
        bin_sort2(m[0], m[1]); bin_sort2(m[3], m[4]); bin_sort2(m[0], m[3]); bin_sort2(m[1], m[4]);
        bin_sort2(m[1], m[2]); bin_sort2(m[2], m[3]); bin_sort2(m[1], m[2]);
        L = m[2];
        leader = (n0 & ((1ll << log2_b) - 1)) == 0;
        if (leader) lv[2 * (size_t)(b & (lv_cap - 1)) + 1] = L;
    }
    int bits = 0;
    if (live && L > 0) {
        int c[8 * sf_components(FMT)], a[8];
        bin_load8<FMT, VEC>(W, n0, c);
        bin_mag8<FMT>(c, a);
        const int lim = threshold_q8 * L;                              // <= 16384 * 65536 = 2^30
#pragma unroll
        for (int j = 0; j < 8; j++) bits |= (256 * a[j] > lim ? 1 : 0) << j;
    }
    if (live) mask[(size_t)((n0 >> 3) & (mask_cap - 1))] = (uint8_t)bits;
    bin_block_sums(__popc(bits), leader && L == 0 && b < cb_end ? 1 : 0, part + 2 * (size_t)blockIdx.x);
}

// The gate of the samples [g0, g1).  Workgroup i owns the 2048 samples from (g0 / 2048 + i) 2048 on = 32 hit words, and reads 2 more on
// either side: sw[k] = word 32 tile - 2 + k of the mask ring, zero outside [m_lo, m_hi) / 64 (the mask is known there; no hit lies
// outside the stream).  The window arithmetic is k_blank_gate's.  Counters: the workgroup's samples with w < 32768 (part[..][0]) and
// with w = 0 (part[..][1]).
template <int FMT, bool VEC>
__global__ __launch_bounds__(BIN_NT) void k_blankin_gate(BinWin W, long long g0, long long g1, long long m_lo, long long m_hi,
                                                         const uint64_t* __restrict__ mask, long long mask_words, int guard, int taper,
                                                         const int32_t* __restrict__ taper_tab, int32_t* __restrict__ part) {
    __shared__ uint64_t sw[40];
    const int tid = threadIdx.x;
    const long long tile = (g0 >> 11) + blockIdx.x, n0 = (tile << 11) + 8 * tid;
    if (tid < 40) {
        const long long w = tile * 32 - 2 + tid;
        sw[tid] = w >= (m_lo >> 6) && w < (m_hi >> 6) ? mask[(size_t)(w & (mask_words - 1))] : 0ull;
    }
    __syncthreads();
    const int q = tid >> 3, s = (tid & 7) * 8;
    uint64_t Wd[5];
#pragma unroll
    for (int k = 0; k < 5; k++) Wd[k] = s ? (sw[q + k] >> s) | (sw[q + k + 1] << (64 - s)) : sw[q + k];
    // any hit at window positions 128 - (guard + taper) .. 135 + guard + taper
    const int lo = BIN_HALO - (guard + taper), hi = BIN_HALO + 7 + guard + taper;
    uint64_t near = 0ull;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const int a = lo > 64 * k ? lo - 64 * k : 0, b = hi < 64 * k + 63 ? hi - 64 * k : 63;
        if (a <= b) near |= Wd[k] & (~0ull >> (63 - b)) & (~0ull << a);
    }
    const bool work = near != 0ull && n0 + 8 > g0 && n0 < g1;
    int n_cut = 0, n_zero = 0;
    if (work) {
        constexpr int NC = sf_components(FMT);
        int c[8 * NC];
        BinWin Wg = W;                                                 // read what is gated, nothing else
        Wg.v0 = g0 > W.v0 ? g0 : W.v0; Wg.v1 = g1 < W.v1 ? g1 : W.v1;
        bin_load8<FMT, VEC>(Wg, n0, c);
        const int32_t* T = taper_tab + taper * BIN_TAPER_ROW;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint64_t at = Wd[2] & ((2ull << j) - 1ull), after = Wd[2] & (~0ull << j);
            // the nearest hit at or before the sample and at or after it, as positions in the window (the sample: 128 + j)
            const int left = at ? 191 - __clzll((long long)at) : Wd[1] ? 127 - __clzll((long long)Wd[1]) : Wd[0] ? 63 - __clzll((long long)Wd[0]) : -1024;
            const int right = after ? 128 + __builtin_ctzll(after) : Wd[3] ? 192 + __builtin_ctzll(Wd[3]) : Wd[4] ? 256 + __builtin_ctzll(Wd[4]) : 2048;
            const int dl = 128 + j - left, dr = right - 128 - j, d = dl < dr ? dl : dr;
            if (d <= guard + taper && n0 + j >= g0 && n0 + j < g1) {
                const int w = d <= guard ? 0 : T[d - guard];
#pragma unroll
                for (int k = 0; k < NC; k++) c[NC * j + k] = (c[NC * j + k] * w + 16384) >> 15;
                n_cut++; n_zero += w == 0;
            }
        }
        bin_store8<FMT, VEC>(W, n0, g0, g1, c);
    }
    bin_block_sums(n_cut, n_zero, part + 2 * (size_t)blockIdx.x);
}

// stats[0 .. 3] += the sums of the partials of one hit launch (n_h workgroups: hits, blocks with L = 0) and one gate launch (n_g: cut,
// zero).  One workgroup; stats is the stream's cumulative int64[4], written by thread 0 alone.
__global__ __launch_bounds__(BIN_NT) void k_blankin_stats(const int32_t* __restrict__ part_h, int n_h, const int32_t* __restrict__ part_g, int n_g,
                                                          long long* __restrict__ stats) {
    __shared__ long long s_sum[4][BIN_NT / 64];
    long long v[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < n_h; i += BIN_NT) { v[0] += part_h[2 * (size_t)i]; v[3] += part_h[2 * (size_t)i + 1]; }
    for (int i = threadIdx.x; i < n_g; i += BIN_NT) { v[1] += part_g[2 * (size_t)i]; v[2] += part_g[2 * (size_t)i + 1]; }
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d);
        if ((threadIdx.x & 63) == 0) s_sum[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < 4; k++) stats[k] += s_sum[k][0] + s_sum[k][1] + s_sum[k][2] + s_sum[k][3];
}
