// Noise blanker (extension; ft8rx_blank*): impulse blanking of 12 kHz int16 frames in place, in integers, so that
// pyft8_amd/blanker.py: reference() gives the same bits.  A frame is 375 blocks of 480 samples; frames are independent.
//   m_b   = element 240 of the sorted |x| of block b                                                  k_blank_level
//   L_b   = element 2 of the sorted m[clamp(b - 2 .. b + 2, 0, 374)]
//   hit   = L_b > 0 and 256 |x[n]| > threshold_q8 L_b                                                 k_blank_hits
//   w[n]  = 0 within `guard` samples of a hit, the raised-cosine table T over the next `taper`, 32768 beyond;
//   y[n]  = (x[n] w[n] + 16384) >> 15                                                                 k_blank_gate
// Three kernels on one stream (and k_blank_stats when the counters are asked for).  k_blank_hits writes the hit flags of EVERY sample
// into a mask of the handle's (one bit per sample, 2813 64-bit words per frame) before k_blank_gate writes the first sample: the gate
// never derives a hit from audio, so a neighbour that has been rewritten already cannot change it, and a thread reads and writes only
// its own 8 samples -- in place is safe.  A thread owns 8 consecutive samples = one 16-byte load / store (8 | 480: a group never
// straddles a block) = one byte of the mask, so the 64-bit words are assembled by byte stores, not by ballots (a ballot would take one
// sample per lane and 2-byte loads).  The gate reads a tile's words and those of its halo (128 samples = 2 words on either side;
// guard + taper <= 128) into LDS, and a thread with no hit within guard + taper of its samples -- nearly all of them -- does not touch
// the audio: a frame without hits is never written.
// Statistics: per-wave integer sums, added up per block through LDS into per-tile partials [frame][88][4] that every block writes in
// full (nothing to clear), and summed by k_blank_stats afterwards: exact, no atomics (one atomicAdd per wave on a frame's four
// counters cost the hit pass 77 us of 101 on 256 impulsive frames).
// VEC = the audio is 16-byte aligned (the staging buffer and every allocation are); otherwise the same groups go by 2-byte accesses.
#pragma once

#define BLK_N 480                      // samples per block
#define BLK_PER_FRAME 375
#define BLK_GROUPS 22500               // groups of 8 samples per frame: a thread each, 60 per block
#define BLK_WORDS 2813                 // 64-bit hit words per frame (the last one half used, its upper half stays zero)
#define BLK_MASK_STRIDE (8 * BLK_WORDS)      // bytes of a frame's hit mask
#define BLK_NT 256
#define BLK_TILES 88                   // blocks of 256 threads x 8 samples per frame (k_blank_hits, k_blank_gate)
#define BLK_HALO 128                   // guard + taper at most
#define BLK_TAPER_ROW 65               // the taper table: row R holds T[1 .. R] of taper = R at [R][1 .. R]

template <bool VEC> FT8_DEV void blk_load8(const int16_t* __restrict__ p, int v[8]) {
    if (VEC) {
        const int4 q = *reinterpret_cast<const int4*>(p);
        const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; i++) { v[2 * i] = (int16_t)(w[i] & 0xffff); v[2 * i + 1] = w[i] >> 16; }
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = p[i];
    }
}
template <bool VEC> FT8_DEV void blk_store8(int16_t* __restrict__ p, const int v[8]) {
    if (VEC) {
        int w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) w[i] = (int)(((uint32_t)v[2 * i] & 0xffffu) | ((uint32_t)v[2 * i + 1] << 16));
        *reinterpret_cast<int4*>(p) = make_int4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) p[i] = (int16_t)v[i];
    }
}
FT8_DEV int blk_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
// the block's sums of a and b -> *pa, *pb.  Every thread of the block calls it (it holds a barrier); thread 0 stores.
FT8_DEV void blk_block_sums(int a, int b, int32_t* __restrict__ pa, int32_t* __restrict__ pb) {
    __shared__ int s_a[BLK_NT / 64], s_b[BLK_NT / 64];
    a = blk_wave_sum(a); b = blk_wave_sum(b);
    if ((threadIdx.x & 63) == 0) { s_a[threadIdx.x >> 6] = a; s_b[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) { *pa = s_a[0] + s_a[1] + s_a[2] + s_a[3]; *pb = s_b[0] + s_b[1] + s_b[2] + s_b[3]; }
}
FT8_DEV void blk_sort2(int& a, int& b) { const int lo = a < b ? a : b, hi = a < b ? b : a; a = lo; b = hi; }

// m_b by exact selection: one wave per block, 8 values per lane (lanes 60 .. 63 hold none).  |x| <= 32768 < 2^16, so 16 steps from bit
// 15 down build the largest r with #{|x| < r} <= 240 = the element at sorted position 240; the counts are popcounts of ballots, uniform
// over the wave (59 us on 256 frames: the scalar unit's popcounts and adds bind it; the lanes' own counts added up through four bit-plane
// ballots instead took 69 us).  x: [n_blocks * 480] (the frames follow each other without a gap: 375 * 480 = 180000); lv: [n_blocks][2], m at [0].
template <bool VEC>
__global__ __launch_bounds__(BLK_NT) void k_blank_level(const int16_t* __restrict__ x, int n_blocks, int32_t* __restrict__ lv) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * (BLK_NT / 64) + (threadIdx.x >> 6);
    if (g >= n_blocks) return;
    int a[8];
    if (lane < BLK_N / 8) {
        blk_load8<VEC>(x + (size_t)g * BLK_N + lane * 8, a);
#pragma unroll
        for (int j = 0; j < 8; j++) a[j] = a[j] < 0 ? -a[j] : a[j];
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) a[j] = 0x7fffffff;
    }
    int r = 0;
#pragma unroll 1
    for (int bit = 15; bit >= 0; bit--) {
        const int c = r | (1 << bit);
        int below = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) below += __popcll(__ballot(a[j] < c));
        if (below <= BLK_N / 2) r = c;
    }
    if (lane == 0) lv[2 * (size_t)g] = r;
}

// Hit flags of every sample, L_b, and the tile's share of the counters `hits` (part[..][0]) and `blocks with L_b = 0` (part[..][3]).
// grid (BLK_TILES, n_frames); thread t of a frame owns samples 8 t .. 8 t + 7 and byte t of the frame's mask, which it always writes.
template <bool VEC>
__global__ __launch_bounds__(BLK_NT) void k_blank_hits(const int16_t* __restrict__ x, int32_t threshold_q8, int32_t* __restrict__ lv,
                                                       uint8_t* __restrict__ mask, int32_t* __restrict__ part) {
    const int f = blockIdx.y, t = blockIdx.x * BLK_NT + threadIdx.x;
    const bool live = t < BLK_GROUPS;
    const int b = live ? t / (BLK_N / 8) : BLK_PER_FRAME - 1;
    int32_t* lvf = lv + 2 * (size_t)f * BLK_PER_FRAME;
    int m[5];
#pragma unroll
    for (int d = 0; d < 5; d++) { int q = b + d - 2; q = q < 0 ? 0 : (q > BLK_PER_FRAME - 1 ? BLK_PER_FRAME - 1 : q); m[d] = lvf[2 * q]; }
    // element 2 of five: after these exchanges m[2] is the median
    blk_sort2(m[0], m[1]); blk_sort2(m[3], m[4]); blk_sort2(m[0], m[3]); blk_sort2(m[1], m[4]);      // m[0] = the smallest, m[4] = the largest
    blk_sort2(m[1], m[2]); blk_sort2(m[2], m[3]); blk_sort2(m[1], m[2]);                            // the middle three in order
    const int L = m[2];
    const bool leader = live && t % (BLK_N / 8) == 0;
    if (leader) lvf[2 * b + 1] = L;
    int bits = 0;
    if (live && L > 0) {
        int v[8];
        blk_load8<VEC>(x + (size_t)f * FT8RX_NSAMP + (size_t)t * 8, v);
        const int lim = threshold_q8 * L;                              // <= 16384 * 32768 = 2^29
#pragma unroll
        for (int j = 0; j < 8; j++) bits |= (256 * (v[j] < 0 ? -v[j] : v[j]) > lim ? 1 : 0) << j;
    }
    if (live) mask[(size_t)f * BLK_MASK_STRIDE + t] = (uint8_t)bits;
    int32_t* pt = part + 4 * ((size_t)f * BLK_TILES + blockIdx.x);
    blk_block_sums(__popc(bits), leader && L == 0 ? 1 : 0, pt + 0, pt + 3);
}

// The gate.  grid (BLK_TILES, n_frames); a block owns 2048 samples = 32 hit words, and reads 2 more on either side.  sw[i] = word
// 32 blockIdx.x - 2 + i of the frame (zero outside the frame: a hit of another frame is never seen).  A thread's window W[0 .. 4] is the
// 320 bits from its first sample - 128 on (a shift by whole bytes of the words in LDS); its samples are bits 128 .. 135.  Distances
// beyond guard + taper give w = 32768 whatever lies there, so nothing has to be cut at guard + taper; a thread with no hit inside
// [first sample - (guard + taper), last sample + guard + taper] leaves the audio alone.  Counters: the tile's samples with w < 32768
// (part[..][1]) and with w = 0 (part[..][2]).
template <bool VEC>
__global__ __launch_bounds__(BLK_NT) void k_blank_gate(int16_t* x, const uint64_t* __restrict__ mask, int guard, int taper,
                                                       const int32_t* __restrict__ taper_tab, int32_t* __restrict__ part) {
    __shared__ uint64_t sw[40];
    const int f = blockIdx.y, tid = threadIdx.x, t = blockIdx.x * BLK_NT + tid;
    if (tid < 40) {
        const int w = blockIdx.x * 32 - 2 + tid;
        sw[tid] = w >= 0 && w < BLK_WORDS ? mask[(size_t)f * BLK_WORDS + w] : 0ull;
    }
    __syncthreads();
    const int q = tid >> 3, s = (tid & 7) * 8;
    uint64_t W[5];
#pragma unroll
    for (int k = 0; k < 5; k++) W[k] = s ? (sw[q + k] >> s) | (sw[q + k + 1] << (64 - s)) : sw[q + k];
    // any hit at window positions 128 - (guard + taper) .. 135 + guard + taper
    const int lo = BLK_HALO - (guard + taper), hi = BLK_HALO + 7 + guard + taper;
    uint64_t near = 0ull;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const int a = lo > 64 * k ? lo - 64 * k : 0, b = hi < 64 * k + 63 ? hi - 64 * k : 63;
        if (a <= b) near |= W[k] & (~0ull >> (63 - b)) & (~0ull << a);
    }
    const bool work = t < BLK_GROUPS && near != 0ull;
    int n_cut = 0, n_zero = 0;
    if (work) {
        int16_t* p = x + (size_t)f * FT8RX_NSAMP + (size_t)t * 8;
        int v[8];
        blk_load8<VEC>(p, v);
        const int32_t* T = taper_tab + taper * BLK_TAPER_ROW;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint64_t at = W[2] & ((2ull << j) - 1ull), after = W[2] & (~0ull << j);
            // the nearest hit at or before the sample and at or after it, as positions in the window (the sample: 128 + j)
            const int left = at ? 191 - __clzll((long long)at) : W[1] ? 127 - __clzll((long long)W[1]) : W[0] ? 63 - __clzll((long long)W[0]) : -1024;
            const int right = after ? 128 + __builtin_ctzll(after) : W[3] ? 192 + __builtin_ctzll(W[3]) : W[4] ? 256 + __builtin_ctzll(W[4]) : 2048;
            const int dl = 128 + j - left, dr = right - 128 - j, d = dl < dr ? dl : dr;
            if (d <= guard + taper) {
                const int w = d <= guard ? 0 : T[d - guard];
                v[j] = (v[j] * w + 16384) >> 15;
                n_cut++; n_zero += w == 0;
            }
        }
        blk_store8<VEC>(p, v);
    }
    int32_t* pt = part + 4 * ((size_t)f * BLK_TILES + blockIdx.x);
    blk_block_sums(n_cut, n_zero, pt + 1, pt + 2);
}

// stats[f][k] = the sum of the frame's 88 tile partials: thread i takes counter i % 4 of frame i / 4
__global__ __launch_bounds__(BLK_NT) void k_blank_stats(const int32_t* __restrict__ part, int n_frames, int32_t* __restrict__ stats) {
    const int i = blockIdx.x * BLK_NT + threadIdx.x;
    if (i >= 4 * n_frames) return;
    const int32_t* p = part + 4 * (size_t)(i >> 2) * BLK_TILES + (i & 3);
    int s = 0;
    for (int t = 0; t < BLK_TILES; t++) s += p[4 * t];
    stats[i] = s;
}
