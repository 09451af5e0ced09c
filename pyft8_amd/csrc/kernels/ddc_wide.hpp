// Wide pre-decimator (extension; ft8rx_ddc_wide*): ONE stream at 240 kHz .. 129.6 MHz -- real int16, IQ int16,
// IQ uint8 (RTL-SDR) or IQ int8 (HackRF) -- -> per channel an IQ float32 stream at the intermediate rate (192 / 96 / 48 kHz), which the
// down-converter of kernels/ddc.hpp takes from there (k_ddc / k_ddc_stream, unchanged).
//   u[n] = x[n] e^{-2 pi i (w0 n mod 2^32) / 2^32}        x = 0 outside the stream
//   v[k] = g0 sum_j h0[j] u[k R0 + j - C0]                = g0 e^{-2 pi i (w0 (k R0 - C0) mod 2^32) / 2^32} sum_j W[j] x[k R0 + j - C0]
//   W[j] = h0[j] e^{-2 pi i (w0 j mod 2^32) / 2^32}       per channel, evaluated in double and rounded once (ft8rx.hip: pre_fill_wide)
// The tile is written once (ddw_tile) and used by two kernels: k_ddc_pre (one call, the input an array) and k_ddc_pre_stream (a
// continuous stream: the input is the history ring and the chunk just pushed).  A block owns `tk` consecutive outputs of one channel
// (blockIdx.y; the channels of a tile run next to each other and share the input in L2).  The taps go by in pieces of DDW_JP: per piece
// the (tk - 1) R0 + DDW_JP input samples under it are loaded coalesced, converted to float and kept in LDS; wave w makes outputs
// w, w + 4, w + 8, w + 12 of the tile, its lane l the taps j = l (mod 64) of all of them in ascending order, so that a table entry
// (read coalesced, out of L2) serves up to four outputs and every LDS read is 64 consecutive samples.  Then a butterfly over the
// lanes.  The order of each sum depends on j and the lane alone: an output is the same bits wherever its tile begins.
// The host side (design of h0, the tables, argument checks, launches, the stream's state) is the one pre-stage path of ft8rx.hip
// (DESIGN.md section 16.4), the index arithmetic in ddc_wide_ring.hpp and ddc_pre_ring.hpp.
#pragma once

#define DDW_NT 256                     // threads per block: 4 waves
#define DDW_JP 1024                    // taps per piece (a multiple of 64: a tap stays with its lane)
#define DDW_LS 6144                    // input samples the LDS image holds: 24 KB real, 48 KB IQ
#define DDW_TK 16                      // outputs per tile at most: 4 per wave
// the wide entries take no float kind (sample_fmt.hpp: SF_KINDS_WIDE): said to the compiler, the loader's float branches are not kept
#define DDW_FORMATS(IQ, fmt) __builtin_assume((IQ) ? (fmt) != SF_IQ_F32 : (fmt) == SF_REAL_I16)

// One tile, the body of k_ddc_pre and of k_ddc_pre_stream: outputs k0 .. k0 + tk - 1 of one channel (tab: its n_taps table entries, w0:
// its frequency word).  load(n) is input sample n, absolute (zero where the stream has none), store(q, v) takes output k0 + q.
// tk <= DDW_TK and (tk - 1) R0 + DDW_JP <= DDW_LS (ddc_wide_ring.hpp: tile_outputs).
template <bool IQ, class Load, class Store>
__device__ __forceinline__ void ddw_tile(const float2* __restrict__ tab, int n_taps, int R0, int tk, uint32_t w0, float g0, long long k0,
                                         Load load, Store store) {
    using S = Sample<IQ>;
    __shared__ typename S::T sx[DDW_LS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, C0 = (n_taps - 1) / 2;
    const long long n0 = k0 * R0 - C0;                // the first input of the tile's first output
    float ar[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ai[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int jp = 0; jp < n_taps; jp += DDW_JP) {
        const int nj = n_taps - jp < DDW_JP ? n_taps - jp : DDW_JP, span = (tk - 1) * R0 + nj;
        if (jp) __syncthreads();                      // the previous piece has been read
        for (int s = t; s < span; s += DDW_NT) sx[s] = load(n0 + jp + s);
        __syncthreads();
        for (int jj = lane; jj < nj; jj += 64) {
            const float2 W = tab[jp + jj];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int q = wave + 4 * i;           // uniform over the wave
                if (q < tk) S::mac(W, sx[q * R0 + jj], ar[i], ai[i]);
            }
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
                // the phase of the output's first input: (k R0 - C0) w0 mod 2^32, in integers
                const uint32_t p = w0 * (uint32_t)(unsigned long long)((k0 + q) * (long long)R0 - C0);
                const float2 v = ddc_cmul(make_float2(ar[i], ai[i]), ddc_phasor(p));
                store(q, make_float2(g0 * v.x, g0 * v.y));
            }
        }
    }
}

// One call: in = n_samples samples of format `fmt`, zero outside -> mid [n_ch][n_mid] (intermediate samples 0 .. n_mid - 1 of every channel)
template <bool IQ>
__global__ __launch_bounds__(DDW_NT) void k_ddc_pre(const void* __restrict__ in, int fmt, long long n_samples, const float2* __restrict__ tab,
                                                    const uint32_t* __restrict__ w0s, int n_taps, int R0, int tk, float g0, long long n_mid,
                                                    float2* __restrict__ mid) {
    DDW_FORMATS(IQ, fmt);
    const int ch = blockIdx.y;
    const long long k0 = (long long)blockIdx.x * tk;
    ddw_tile<IQ>(tab + (size_t)ch * n_taps, n_taps, R0, tk, w0s[ch], g0, k0, ArrayLoad<IQ>{in, fmt, n_samples},
                 [&](int q, float2 v) { if (k0 + q < n_mid) mid[(size_t)ch * (size_t)n_mid + (size_t)(k0 + q)] = v; });
}

// The stream (ft8rx_ddc_wide_stream_push): intermediate samples k_first .. k_first + n_k - 1 of every channel -> mid [n_ch][n_k].  The
// input is the history ring and the chunk of this push (kernels/sample.hpp: StreamLoad).
template <bool IQ>
__global__ __launch_bounds__(DDW_NT) void k_ddc_pre_stream(const void* __restrict__ hist, int H, int p_last, const void* __restrict__ chunk, int fmt,
                                                           long long n_origin, long long n_start, long long n_end, const float2* __restrict__ tab,
                                                           const uint32_t* __restrict__ w0s, int n_taps, int R0, int tk, float g0,
                                                           long long k_first, int n_k, float2* __restrict__ mid) {
    DDW_FORMATS(IQ, fmt);
    const int ch = blockIdx.y;
    const long long k0 = k_first + (long long)blockIdx.x * tk;
    ddw_tile<IQ>(tab + (size_t)ch * n_taps, n_taps, R0, tk, w0s[ch], g0, k0, StreamLoad<IQ>{hist, H, p_last, chunk, fmt, n_origin, n_start, n_end},
                 [&](int q, float2 v) {
                     const long long kk = (long long)blockIdx.x * tk + q;
                     if (kk < n_k) mid[(size_t)ch * (size_t)n_k + (size_t)kk] = v;
                 });
}
