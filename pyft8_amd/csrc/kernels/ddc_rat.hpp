// Rational resampler (extension; ft8rx_ddc_rat*): ONE stream at a rate that is rate_mid M / L with L > 1 (44.1 kHz
// sound cards, RTL-SDR at 2.048 MS/s, HackRF at 10 MS/s) -- real int16 / float32, IQ int16 / float32 / uint8 / int8 -- -> per channel an
// IQ float32 stream at the intermediate rate (192 / 96 / 48 kHz), which the down-converter of kernels/ddc.hpp takes from there (k_ddc /
// k_ddc_stream, unchanged).  With the prototype h (N taps, odd, C = (N - 1) / 2, sum h = L) and t_k = k M + C:
//   u[n] = x[n] e^{-2 pi i (w0 n mod 2^32) / 2^32}                                  x = 0 outside the stream
//   v[k] = g0 sum_{0 <= j < N, j = t_k (mod L)} h[j] u[(t_k - j) / L]
//        = g0 e^{-2 pi i (w0 b_k mod 2^32) / 2^32} sum_{i < P} T[phi_k][i] x[b_k - i]     b_k = t_k / L, phi_k = t_k mod L, P = ceil(N / L)
//   T[phi][i] = h[phi + i L] e^{+2 pi i (w0 i mod 2^32) / 2^32}                      per channel, zero from N on, evaluated in double and
//                                                                                  rounded once (ft8rx.hip: pre_fill_rat)
// All index arithmetic is in 64-bit integers (n < 2^52, L <= 320).  The tile is written once (ddr_tile) and used by two kernels:
// k_ddc_rat (one call, the input an array) and k_ddc_rat_stream (a continuous stream: the input is the history ring and the chunk just
// pushed).  A block owns `tk` consecutive outputs of one channel (blockIdx.y).  Two regimes, a property of the rate alone
// (ddc_rat_ring.hpp: lane_regime):
//   LANE  (P <= 64 and the table fits: 44.1 kHz P = 7, 250 kHz 33, 2.048 MHz 60)  the channel's table [L][P] and the input under the
//         tile's outputs are staged in LDS once; lane q makes output k0 + q, summing i = 0 .. P - 1 in ascending order.
//   WAVE  (1 MS/s P = 130, 10 MS/s 1291)  the wide kernel's scheme: the taps go by in pieces of DDR_JP, per piece the input under it is
//         kept in LDS (newest first, so that a lane's reads run with its taps); wave w makes outputs w, w + 4, w + 8, w + 12 of the tile,
//         its lane l the taps i = l (mod 64) in ascending order; then a butterfly over the lanes.
// The order of an output's sum depends on the plan, phi_k, i and the lane alone: an output is the same bits wherever its tile or its
// chunk begins.  The host side (design of h, the tables, argument checks, launches, the stream's state) is the one pre-stage path of
// ft8rx.hip, the index arithmetic in ddc_rat_ring.hpp and ddc_pre_ring.hpp.
#pragma once

#define DDR_NT 256                     // threads per block: 4 waves
#define DDR_TAB 3072                   // LANE: table entries in LDS (24 KB)
#define DDR_LS_LANE 3200               // LANE: input samples in LDS next to the table
#define DDR_JP 1024                    // WAVE: taps per piece (a multiple of 64: a tap stays with its lane)
#define DDR_LS_WAVE 6144               // WAVE: input samples the LDS image holds
#define DDR_TK_WAVE 16                 // WAVE: outputs per tile at most, 4 per wave

template <bool IQ, bool LANE> struct DdrLds {
    typedef typename Sample<IQ>::T T;
    static constexpr int BYTES = LANE ? (int)sizeof(float2) * DDR_TAB + (int)sizeof(T) * DDR_LS_LANE : (int)sizeof(T) * DDR_LS_WAVE;
};

// One tile, the body of k_ddc_rat and of k_ddc_rat_stream: outputs k0 .. k0 + tk - 1 of one channel (tab: its table [L][P], w0: its
// frequency word; C = (N - 1) / 2).  load(n) is input sample n, absolute (zero where the stream has none), store(q, v) takes output
// k0 + q.  tk = ddc_rat_ring.hpp: tile_outputs, so that the inputs under the tile fit the LDS image.
template <bool IQ, bool LANE, class Load, class Store>
__device__ __forceinline__ void ddr_tile(const float2* __restrict__ tab, int C, int L, int M, int P, int tk, uint32_t w0, float g0, long long k0,
                                         Load load, Store store) {
    using S = Sample<IQ>;
    typedef typename S::T T;
    __shared__ __align__(16) unsigned char smem[DdrLds<IQ, LANE>::BYTES];
    const int t = threadIdx.x;
    // the last inputs of the tile's first and last output
    const long long b_lo = (k0 * M + C) / L, b_hi = ((k0 + tk - 1) * M + C) / L;
    if constexpr (LANE) {
        float2* st = (float2*)smem;
        T* sx = (T*)(smem + sizeof(float2) * DDR_TAB);
        const long long n_lo = b_lo - (P - 1);
        const int span = (int)(b_hi - n_lo) + 1;      // <= DDR_LS_LANE
        for (int s = t; s < L * P; s += DDR_NT) st[s] = tab[s];
        for (int s = t; s < span; s += DDR_NT) sx[s] = load(n_lo + s);
        __syncthreads();
        if (t < tk) {
            const long long tq = (k0 + t) * M + C, b = tq / L;
            const float2* W = st + (int)(tq - b * L) * P;
            const T* x = sx + (int)(b - n_lo);
            float ar = 0.0f, ai = 0.0f;
            for (int i = 0; i < P; i++) S::mac(W[i], x[-i], ar, ai);
            // the phase of the output's last input: b w0 mod 2^32, in integers
            const float2 v = ddc_cmul(make_float2(ar, ai), ddc_phasor(w0 * (uint32_t)(unsigned long long)b));
            store(t, make_float2(g0 * v.x, g0 * v.y));
        }
    } else {
        T* sx = (T*)smem;
        const int lane = t & 63, wave = t >> 6;
        float ar[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ai[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        long long b[4]; int back[4], row[4];          // uniform over the wave: last input, its distance from b_hi, the table row
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int q = wave + 4 * i < tk ? wave + 4 * i : tk - 1;
            const long long tq = (k0 + q) * M + C;
            b[i] = tq / L; back[i] = (int)(b_hi - b[i]); row[i] = (int)(tq - b[i] * L) * P;
        }
        for (int ip = 0; ip < P; ip += DDR_JP) {
            const int ni = P - ip < DDR_JP ? P - ip : DDR_JP, span = (int)(b_hi - b_lo) + ni;      // <= DDR_LS_WAVE
            if (ip) __syncthreads();                  // the previous piece has been read
            for (int s = t; s < span; s += DDR_NT) sx[s] = load(b_hi - ip - s);      // newest first: sx[s] is input b_hi - ip - s
            __syncthreads();
            for (int jj = lane; jj < ni; jj += 64) {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (wave + 4 * i < tk) S::mac(tab[row[i] + ip + jj], sx[back[i] + jj], ar[i], ai[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
            for (int off = 32; off; off >>= 1) { ar[i] += __shfl_xor(ar[i], off); ai[i] += __shfl_xor(ai[i], off); }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int q = wave + 4 * i;
                if (q < tk) {
                    const float2 v = ddc_cmul(make_float2(ar[i], ai[i]), ddc_phasor(w0 * (uint32_t)(unsigned long long)b[i]));
                    store(q, make_float2(g0 * v.x, g0 * v.y));
                }
            }
        }
    }
}

// One call: in = n_samples samples of format `fmt`, zero outside -> mid [n_ch][n_mid] (intermediate samples 0 .. n_mid - 1 of every channel)
template <bool IQ, bool LANE>
__global__ __launch_bounds__(DDR_NT) void k_ddc_rat(const void* __restrict__ in, int fmt, long long n_samples, const float2* __restrict__ tab,
                                                    const uint32_t* __restrict__ w0s, int C, int L, int M, int P, int tk, float g0, long long n_mid,
                                                    float2* __restrict__ mid) {
    const int ch = blockIdx.y;
    const long long k0 = (long long)blockIdx.x * tk;
    ddr_tile<IQ, LANE>(tab + (size_t)ch * (size_t)(L * P), C, L, M, P, tk, w0s[ch], g0, k0, ArrayLoad<IQ>{in, fmt, n_samples},
                       [&](int q, float2 v) { if (k0 + q < n_mid) mid[(size_t)ch * (size_t)n_mid + (size_t)(k0 + q)] = v; });
}

// The stream (ft8rx_ddc_rat_stream_push): intermediate samples k_first .. k_first + n_k - 1 of every channel -> mid [n_ch][n_k].  The
// input is the history ring and the chunk of this push (kernels/sample.hpp: StreamLoad).
template <bool IQ, bool LANE>
__global__ __launch_bounds__(DDR_NT) void k_ddc_rat_stream(const void* __restrict__ hist, int H, int p_last, const void* __restrict__ chunk, int fmt,
                                                           long long n_origin, long long n_start, long long n_end, const float2* __restrict__ tab,
                                                           const uint32_t* __restrict__ w0s, int C, int L, int M, int P, int tk, float g0,
                                                           long long k_first, int n_k, float2* __restrict__ mid) {
    const int ch = blockIdx.y;
    const long long k0 = k_first + (long long)blockIdx.x * tk;
    ddr_tile<IQ, LANE>(tab + (size_t)ch * (size_t)(L * P), C, L, M, P, tk, w0s[ch], g0, k0,
                       StreamLoad<IQ>{hist, H, p_last, chunk, fmt, n_origin, n_start, n_end},
                       [&](int q, float2 v) {
                           const long long kk = (long long)blockIdx.x * tk + q;
                           if (kk < n_k) mid[(size_t)ch * (size_t)n_k + (size_t)kk] = v;
                       });
}
