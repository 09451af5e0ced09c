// Down-converter (extension; ft8rx_ddc): real or IQ input at 12 D kHz -> the 12 kHz USB audio frames the decode
// path takes.  One fused kernel per output tile: load + mix -> LDS, stage 1 (rate -> 24 kHz) out of LDS into a second LDS image,
// stage 2 (24 -> 12 kHz) out of that image, +3000 Hz shift, real part, int16 (and optionally the float32 value before rounding).
//   u[n] = x[n] e^{-2 pi i (w n mod 2^32) / 2^32}         x = 0 outside [0, n_samples)
//   v[k] = sum_j h1[j] u[k R1 + j - C1]                   D >= 4 only (R1 = D / 2); otherwise v = u
//   z[m] = sum_j h2[j] v[m R2 + j - C2]                   R2 = 2 (1 at D = 1)
//   y[m] = scale Re(i^m z[m])                             scale = gain sf_real_gain(fmt)
// The tile is written once (ddc_tile) and used by two kernels: k_ddc (one call = one cycle, the input an array of the call) and
// k_ddc_stream (a continuous stream, the input a ring of the newest samples, the output a ring of two cycles,
// indices absolute); k_ddc_gather cuts frames out of that ring.
// The host side (design of the taps, argument checks, launch, the stream's state) is in ft8rx.hip, the stream's index arithmetic in
// ddc_ring.hpp.
#pragma once

#define DDC_NT 256                     // threads per block
#define DDC_TO 1008                    // outputs per tile: a multiple of 4 (the i^m pattern starts over in every tile) with
                                       // 2 DDC_TO + 281 = 2297 just under 9 x 256 (stage 1 makes 256 samples of v per chunk)
#define DDC_TILES ((FT8RX_NSAMP + DDC_TO - 1) / DDC_TO)
#define DDC_QN 128                     // entries of the per-tile phasor table (step 256 samples)

// The taps: float32, rounded once from the double design (ft8rx.hip: ddc_design), uploaded at the handle's first ft8rx_ddc.  The tap
// index is uniform over a wave, so the loads are scalar.
__constant__ float c_ddc_h1[3][64];    // stage 1 at D = 4, 8, 16: 17, 31, 61 taps
__constant__ float c_ddc_h2[2][288];   // stage 2: [0] 283 taps at 24 kHz, [1] 143 taps at 12 kHz (D = 1)

struct DdcOut { int32_t src, out; uint32_t w, pad; };      // one output channel: its stream, its frame in the output, its frequency word

template <int D> struct DdcGeom {
    static constexpr int R1 = D >= 4 ? D / 2 : 1;                          // stage 1 decimation
    static constexpr int N1 = D == 4 ? 17 : D == 8 ? 31 : D == 16 ? 61 : 1;
    static constexpr int C1 = (N1 - 1) / 2;
    static constexpr int H1 = D == 4 ? 0 : D == 8 ? 1 : 2;                 // row of c_ddc_h1
    static constexpr int R2 = D == 1 ? 1 : 2;
    static constexpr int N2 = D == 1 ? 143 : 283;
    static constexpr int C2 = (N2 - 1) / 2;
    static constexpr int NV = (DDC_TO - 1) * R2 + N2;                      // samples of v a tile needs
    static constexpr int NCH = (NV + DDC_NT - 1) / DDC_NT;                 // stage-1 chunks of 256 v samples
    static constexpr int LU = (DDC_NT - 1) * R1 + N1;                      // input samples under one chunk
    // the chunk's input in LDS, one row per polyphase branch (input index mod R1): lane t reads row j % R1 at t + j / R1, stride 1.
    // BL = 32 / R1 (mod 32) spreads the 32 float2 a half wave WRITES (R1 rows x 32 / R1 columns) over all 64 banks.
    static constexpr int BL = R1 == 2 ? 272 : R1 == 4 ? 264 : 292;
    // the v image: one float array per component (re, im) and, at R2 = 2, per parity of the index.  Lane t of stage 2 reads array
    // (t & 1, j & 1) at o + j / 2: the component alternates with the lane, so 2 S = 0 (mod 64) keeps a wave's 64 reads on 64 banks; the
    // parity alternates with the lane when stage 1 writes, so S = 32 (mod 64) does the same there.
    static constexpr int S = R2 == 2 ? 1184 : 1216;
    static constexpr int VF = R2 == 2 ? 4 * S : 2 * S;
    static_assert(R2 == 1 || (NV + 1) / 2 <= S, "v image: a parity row holds the tile");
    static_assert(4 * DDC_NT - 1 + (N2 - 1) / R2 < S, "v image: the last lane's last read stays inside its row");
    static_assert(R1 == 1 || (LU - 1) / R1 < BL, "input chunk: a branch row holds the chunk");
    static_assert(NCH * R1 + (LU + DDC_NT - 1) / DDC_NT <= DDC_QN && NCH <= DDC_QN, "phasor table");
    static_assert(DDC_TO % 4 == 0 && DDC_TO <= 4 * DDC_NT, "tile");
};

// e^{-2 pi i p / 2^32}: evaluated in double, rounded once
__device__ __forceinline__ float2 ddc_phasor(uint32_t p) {
    double s, c;
    sincospi(-(double)p * (1.0 / 2147483648.0), &s, &c);
    return make_float2((float)c, (float)s);
}
__device__ __forceinline__ float2 ddc_cmul(float2 a, float2 b) {
    return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}
// sample i of an array of format `fmt` as a complex float
__device__ __forceinline__ float2 ddc_fetch(const void* __restrict__ in, int fmt, size_t i) {
    __builtin_assume(fmt >= SF_REAL_I16 && fmt <= SF_IQ_F32);      // what ddc_check lets through: no 8-bit branch is kept
    return sf_is_iq(fmt) ? Sample<true>::fetch(in, fmt, i) : make_float2(Sample<false>::fetch(in, fmt, i), 0.0f);
}

// One output tile, the body of k_ddc and of k_ddc_stream: load + mix -> LDS, stage 1 -> the v image, stage 2, i^m, scale.  The tile's
// first output index is a multiple of 4 and its first input is n0; only n0 mod 2^32 (p0) enters the phase.  load(i) is input sample
// n0 + i (zero where the stream has none), store(o, y) takes output o of the tile, o < DDC_TO, before rounding.
template <int D, class Load, class Store>
__device__ __forceinline__ void ddc_tile(uint32_t w, uint32_t p0, float scale, Load load, Store store) {
    using G = DdcGeom<D>;
    constexpr int R1 = G::R1, N1 = G::N1, R2 = G::R2, N2 = G::N2, S = G::S, BL = G::BL;
    __shared__ float sv[G::VF];
    __shared__ float2 su[R1 > 1 ? R1 * BL : 1];
    __shared__ float2 sq[DDC_QN];
    const int t = threadIdx.x;
    // phase of input n0 + t + 256 e = phase(n0 + t) + phase(256 e), integers mod 2^32: one phasor per thread, one table per tile
    const float2 P = ddc_phasor(w * (p0 + (uint32_t)t));
    if (t < DDC_QN) sq[t] = ddc_phasor(w * (uint32_t)(DDC_NT * t));
    __syncthreads();

    auto store_v = [&](int i, float2 v) {
        if constexpr (R2 == 2) { sv[(i & 1) * S + (i >> 1)] = v.x; sv[(2 + (i & 1)) * S + (i >> 1)] = v.y; }
        else { sv[i] = v.x; sv[S + i] = v.y; }
    };
    if constexpr (R1 == 1) {                          // no stage 1: the mixed input is v
        for (int i = t; i < G::NV; i += DDC_NT)
            store_v(i, ddc_cmul(load(i), ddc_cmul(P, sq[i / DDC_NT])));
    } else {
        const float* h1 = c_ddc_h1[G::H1];
        for (int c = 0; c < G::NCH; c++) {
            const int nb = DDC_NT * R1 * c;           // first input under the chunk, from n0
            if (c) __syncthreads();                   // the previous chunk has been read
            for (int e = 0; e * DDC_NT < G::LU; e++) {
                const int l = t + DDC_NT * e;
                if (l < G::LU)
                    su[(l % R1) * BL + l / R1] = ddc_cmul(load(nb + l), ddc_cmul(P, sq[e + R1 * c]));
            }
            __syncthreads();
            const int i = c * DDC_NT + t;
            if (i < G::NV) {
                float ar = 0.0f, ai = 0.0f;
#pragma unroll
                for (int j = 0; j < N1; j++) {
                    const float2 u = su[(j % R1) * BL + t + j / R1];
                    ar = fmaf(h1[j], u.x, ar); ai = fmaf(h1[j], u.y, ai);
                }
                store_v(i, make_float2(ar, ai));
            }
        }
    }
    __syncthreads();

    // stage 2: outputs o = t + 256 q.  Re(i^m z) is +re, -im, -re, +im of z for m = 0, 1, 2, 3 (mod 4), and the tile starts at a
    // multiple of 4: a lane needs one component only, the same for its four outputs
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (R2 == 2) {
        const float* h2 = c_ddc_h2[0];
        const float* b = sv + (t & 1) * 2 * S + t;
#pragma unroll 4
        for (int jj = 0; jj < N2 / 2; jj++) {         // taps 2 jj (even index of v) and 2 jj + 1 (odd)
            const float he = h2[2 * jj], ho = h2[2 * jj + 1];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                acc[q] = fmaf(he, b[jj + DDC_NT * q], acc[q]);
                acc[q] = fmaf(ho, b[S + jj + DDC_NT * q], acc[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = fmaf(h2[N2 - 1], b[N2 / 2 + DDC_NT * q], acc[q]);
    } else {
        const float* h2 = c_ddc_h2[1];
        const float* b = sv + (t & 1) * S + t;
#pragma unroll 8
        for (int j = 0; j < N2; j++) {
            const float hj = h2[j];
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] = fmaf(hj, b[j + DDC_NT * q], acc[q]);
        }
    }
    const float sg = ((t & 3) == 0 || (t & 3) == 3) ? scale : -scale;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int oo = t + DDC_NT * q;
        if (oo < DDC_TO) store(oo, sg * acc[q]);
    }
}
__device__ __forceinline__ int16_t ddc_round(float y) { return (int16_t)fminf(fmaxf(rintf(y), -32768.0f), 32767.0f); }

template <int D>
__global__ __launch_bounds__(DDC_NT) void k_ddc(const void* __restrict__ in, int fmt, unsigned long long stream_stride, int n_samples,
                                                const DdcOut* __restrict__ outs, float scale, int16_t* __restrict__ audio,
                                                float* __restrict__ audio_f32) {
    using G = DdcGeom<D>;
    // stream-major: the blocks of one output follow each other, outputs sorted by stream (outs is in that order)
    const DdcOut o = outs[blockIdx.x / DDC_TILES];
    const int m0 = (int)(blockIdx.x % DDC_TILES) * DDC_TO;
    const int k0 = m0 * G::R2 - G::C2;                // first v index of the tile
    const int n0 = k0 * G::R1 - G::C1;                // first input index of the tile (negative in the first tile)
    const size_t base = (size_t)o.src * (size_t)stream_stride;
    ddc_tile<D>(o.w, (uint32_t)n0, scale,
                [&](int i) {                          // the input is zero outside [0, n_samples)
                    const int n = n0 + i;
                    return n < 0 || n >= n_samples ? make_float2(0.0f, 0.0f) : ddc_fetch(in, fmt, base + (size_t)n);
                },
                [&](int oo, float y) {
                    const int m = m0 + oo;
                    if (m >= FT8RX_NSAMP) return;
                    const size_t at = (size_t)o.out * FT8RX_NSAMP + (size_t)m;
                    if (audio_f32) audio_f32[at] = y;
                    audio[at] = ddc_round(y);
                });
}

// The streaming down-converter (ft8rx_ddc_stream_push): the same tile on a continuous stream.  Indices are
// absolute and 64 bit: tile `tile` holds the outputs m = DDC_TO tile + o.  Its input comes out of the stream's ring of the newest
// `cap` samples (a power of two; sample n at (n - n_origin) & (cap - 1)), zero before the origin n_origin (and from n_end on, which
// no complete tile reaches); its output goes to the channel's ring at m mod ring_len.  One block per (channel, new tile).
template <int D>
__global__ __launch_bounds__(DDC_NT) void k_ddc_stream(const void* __restrict__ ring_in, int fmt, unsigned long long cap, long long n_origin,
                                                       long long n_end, const DdcOut* __restrict__ outs, long long tile_first, int n_tiles,
                                                       float scale, int ring_len, int16_t* __restrict__ ring_out, float* __restrict__ ring_f32) {
    using G = DdcGeom<D>;
    const DdcOut o = outs[blockIdx.x / n_tiles];
    const long long m0 = (tile_first + (long long)(blockIdx.x % n_tiles)) * DDC_TO;
    const long long n0 = (m0 * G::R2 - G::C2) * G::R1 - G::C1;
    const size_t base = (size_t)o.src * (size_t)cap;
    const int r0 = (int)(m0 % ring_len);              // m0 >= 0: the origin is not negative
    const size_t row = (size_t)o.out * (size_t)ring_len;
    ddc_tile<D>(o.w, (uint32_t)(unsigned long long)n0, scale,
                [&](int i) {
                    const long long n = n0 + i;
                    return n < n_origin || n >= n_end ? make_float2(0.0f, 0.0f)
                                                      : ddc_fetch(ring_in, fmt, base + (size_t)((unsigned long long)(n - n_origin) & (cap - 1)));
                },
                [&](int oo, float y) {
                    int r = r0 + oo;
                    if (r >= ring_len) r -= ring_len;
                    if (ring_f32) ring_f32[row + r] = y;
                    ring_out[row + r] = ddc_round(y);
                });
}

// ft8rx_ddc_stream_frame: frame j position p = output m_first + p of channel j out of its ring; zero from n_have on and where the
// stream has no output (before m_origin, from m_done on)
template <class S>
FT8_DEV void ddc_gather(const S* __restrict__ ring, int ring_len, long long m_first, int n_have, long long m_origin, long long m_done,
                        S* __restrict__ audio) {
    const int p = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (p >= FT8RX_NSAMP) return;
    const long long m = m_first + p;
    S v = 0;
    if (p < n_have && m >= m_origin && m < m_done) v = ring[(size_t)j * ring_len + (size_t)(m % ring_len)];
    audio[(size_t)j * FT8RX_NSAMP + p] = v;
}
__global__ __launch_bounds__(256) void k_ddc_gather(const int16_t* __restrict__ ring, int ring_len, long long m_first, int n_have,
                                                    long long m_origin, long long m_done, int16_t* __restrict__ audio) {
    ddc_gather(ring, ring_len, m_first, n_have, m_origin, m_done, audio);
}
// ft8rx_ddc_stream_frame_f32: the same cut of the float32 output ring, the same zero rules
__global__ __launch_bounds__(256) void k_ddc_gather_f32(const float* __restrict__ ring, int ring_len, long long m_first, int n_have,
                                                        long long m_origin, long long m_done, float* __restrict__ audio) {
    ddc_gather(ring, ring_len, m_first, n_have, m_origin, m_done, audio);
}
// ft8rx_ddc_stream_frames: frame i position p = output m_first + p of channel sel[i], for frames of frame_len
// samples (a 15-s or a 7.5-s frame), the zero rules of k_ddc_gather.  sel: the stream's table of the call's channel list, checked on
// the host (ddc_frames.hpp); an entry outside [0, n_out) reads nothing, so no load leaves a ring row
__global__ __launch_bounds__(256) void k_ddc_gather_sel(const int16_t* __restrict__ ring, int ring_len, const int32_t* __restrict__ sel, int n_out,
                                                        long long m_first, int n_have, long long m_origin, long long m_done, int frame_len,
                                                        int16_t* __restrict__ audio) {
    const int p = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (p >= frame_len) return;
    const int j = sel[i];
    const long long m = m_first + p;
    int16_t v = 0;
    if (p < n_have && m >= m_origin && m < m_done && (unsigned)j < (unsigned)n_out) v = ring[(size_t)j * ring_len + (size_t)(m % ring_len)];
    audio[(size_t)i * frame_len + p] = v;
}
