// Panorama (extension; ft8rx_pan*): the averaged power spectrum of ONE raw input stream at its own rate, and
// the count of samples at the converter's rails.  pyft8_amd/pan.py: reference() is the float64 twin.
//   v      = the sample on the int16 scale (kernels/sample.hpp), a real kind with zero imaginary part
//   X_w[k] = sum_i win[i] v[w N + i] e^(-2 pi i ik / N), window w = the ABSOLUTE samples [w N, (w + 1) N), a float32 FFT     k_pan_power
//   p_w[j] = Re^2 + Im^2 of bin k(j): IQ kinds j = 0 .. N - 1, k = (j + N / 2) mod N; real kinds j = k = 0 .. N / 2 - 1
//   P_r[j] = ((p_{rA}[j] + p_{rA + 1}[j]) + p_{rA + 2}[j]) + ..., the A windows of row r in WINDOW ORDER, float32               k_pan_rows
// A real kind is transformed as a complex sequence with zero imaginary part: one arithmetic for both, the twin's.
//
// k_pan_power: one workgroup per window.  The window lives in LDS as two float arrays (re, im: every access is 4 bytes wide, bank =
// word mod 32 within a 32-lane half); a pass reads all its butterflies into registers, a barrier, then writes them back IN PLACE, so
// N = 8192 takes 64 KB.  Pass (n, s, R): butterfly b = p s + q reads the elements b + j N / R -- 32 consecutive words per half-wave,
// conflict-free -- and writes q + s (R p + j), which for s < 32 strides over the banks.  Each pass therefore stores through its own
// XOR swizzle pan_swz<log2 s, log2 R>: it moves the lane bits that the stride pushed above bit 4 into the bank bits the constant j
// left free, inside each aligned run of 32 words, so the next pass's reads of aligned runs stay conflict-free and the writes become
// so.  The last pass (s = N / R) needs no store: its outputs are the bins b + j N / R, written to global memory as powers.
// k_pan_rows: thread (row, bin) adds the windows of its row that this launch holds, in window order, on top of what the row's ring
// slot holds from the launches before (a row in progress accumulates in its own slot); one more workgroup per row sums the windows'
// statistics.  The order of the additions is the window's position in its row, whatever the cut into pushes and tiles.
// Statistics: per window (samples with a component at a rail, largest |c| in the blanker's units), from the exact float values;
// every workgroup writes its own pair, k_pan_rows adds them: exact, no atomics.
#pragma once

#define PAN_TW_N 8192                          // the twiddle table: W_8192^k, k < 8192; W_N^k = entry k (8192 / N)
#define PAN_ROWS_NT 128                        // threads of k_pan_rows: every bin count (128 .. 8192) is a multiple

constexpr int pan_log2(int n) { return n <= 1 ? 0 : 1 + pan_log2(n / 2); }
constexpr int pan_nt(int N) { return N / 16 < 64 ? 64 : N / 16 > 256 ? 256 : N / 16; }
// radix of the pass that has n elements per sub-transform left: 8, and 4 where a multiple of 8 would leave 2
constexpr int pan_radix(int n) { return n == 4 || n == 16 ? 4 : 8; }

// the swizzle of a buffer written by pass (s = 2^a, R = 2^r): word i -> i ^ (bits [sh, sh + cnt) of i, moved to [a, a + cnt)), with
// sh = max(a, 5 - r) + r >= 5 and a + cnt <= 5: a bijection of every aligned 32-word run onto itself
template <int a, int r> FT8_DEV int pan_swz(int i) {
    if constexpr (a >= 5) return i;
    else {
        constexpr int cnt = 5 - a < r ? 5 - a : r, sh = (a > 5 - r ? a : 5 - r) + r;
        return i ^ (((i >> sh) & ((1 << cnt) - 1)) << a);
    }
}

// sample i of the window at x: ALIGNED = x is aligned to a sample (the one loader of kernels/sample.hpp); otherwise to a component
// only, and the components are fetched one by one
FT8_DEV float pan_component(const void* __restrict__ in, int fmt, size_t c) {
    if (fmt == SF_REAL_I16 || fmt == SF_IQ_I16) return (float)((const int16_t*)in)[c];
    if (fmt == SF_REAL_F32 || fmt == SF_IQ_F32) return ((const float*)in)[c];
    if (fmt == SF_IQ_U8) return (float)(256 * (int)((const uint8_t*)in)[c] - 32640);
    return (float)(256 * (int)((const int8_t*)in)[c]);
}
template <bool IQ, bool ALIGNED> FT8_DEV cpx pan_fetch(const void* __restrict__ in, int fmt, size_t i) {
    if constexpr (IQ) {
        if constexpr (ALIGNED) return Sample<true>::fetch(in, fmt, i);
        else return make_float2(pan_component(in, fmt, 2 * i), pan_component(in, fmt, 2 * i + 1));
    } else {
        return make_float2(ALIGNED ? Sample<false>::fetch(in, fmt, i) : pan_component(in, fmt, i), 0.0f);
    }
}
// rail and |c| of one component value v (exact in float32): int16 codes -32768 / 32767, c = v; int8 v = 256 s; uint8 v = 256 u - 32640,
// c = 2 u - 255 = v / 128; float kinds have no rails
FT8_DEV void pan_rail(float v, int fmt, int& rail, int& peak) {
    if (fmt == SF_REAL_F32 || fmt == SF_IQ_F32) return;
    const int c = (int)v, lo = fmt == SF_IQ_U8 ? -32640 : -32768, hi = fmt == SF_IQ_U8 ? 32640 : fmt == SF_IQ_I8 ? 32512 : 32767;
    const int m = (c < 0 ? -c : c) >> (fmt == SF_IQ_U8 ? 7 : fmt == SF_IQ_I8 ? 8 : 0);
    rail |= c == lo || c == hi ? 1 : 0;
    peak = m > peak ? m : peak;
}

// The passes from (n, s) on, each in place over the window in LDS.  PA, PR: log2 s and log2 R of the pass that wrote the buffer, whose
// swizzle the reads undo (5, 0 for the load, which stores word i at i).  The last pass writes the powers to `out` in output order.
template <int N, int n, int s, int PA, int PR, bool IQ>
FT8_DEV void pan_passes(float* __restrict__ s_re, float* __restrict__ s_im, const cpx* __restrict__ tw, float* __restrict__ out, int tid) {
    constexpr int R = pan_radix(n), m = n / R, NB = N / R, NT = pan_nt(N), PER = (NB + NT - 1) / NT;
    constexpr int a = pan_log2(s), r = pan_log2(R);
    cpx v[PER][R];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int b = tid + u * NT;
        if (NB % NT == 0 || b < NB) {
#pragma unroll
            for (int j = 0; j < R; j++) { const int i = pan_swz<PA, PR>(b + j * NB); v[u][j] = make_float2(s_re[i], s_im[i]); }
        }
    }
    if constexpr (m > 1) __syncthreads();                              // every butterfly is in registers before any is written back
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int b = tid + u * NT;
        if (NB % NT == 0 || b < NB) {
            const int p = b / s, q = b - p * s;
            dft<R>(v[u]);
            if constexpr (m > 1) {
#pragma unroll
                for (int j = 0; j < R; j++) {
                    const cpx y = j ? cmul(v[u][j], tw[(j * p * s) * (PAN_TW_N / N)]) : v[u][0];
                    const int i = pan_swz<a, r>(q + s * (R * p + j));
                    s_re[i] = y.x; s_im[i] = y.y;
                }
            } else {                                                   // the last pass: bin k = b + j N / R
#pragma unroll
                for (int j = 0; j < R; j++) {
                    const int k = b + j * NB;
                    const float pw = v[u][j].x * v[u][j].x + v[u][j].y * v[u][j].y;
                    if (IQ) out[(k + N / 2) & (N - 1)] = pw;
                    else if (k < N / 2) out[k] = pw;
                }
            }
        }
    }
    if constexpr (m > 1) {
        __syncthreads();
        pan_passes<N, m, s * R, a, r, IQ>(s_re, s_im, tw, out, tid);
    }
}

// window blockIdx.x of the launch: x = its first window's first sample, win = the N weights, pw [windows][bins], wstat [windows][2]
template <int N, bool IQ, bool ALIGNED>
__global__ __launch_bounds__(pan_nt(N)) void k_pan_power(const char* __restrict__ x, int fmt, const float* __restrict__ win, const cpx* __restrict__ tw,
                                                         float* __restrict__ pw, int32_t* __restrict__ wstat) {
    constexpr int NT = pan_nt(N), BINS = IQ ? N : N / 2;
    __shared__ float s_re[N], s_im[N];
    __shared__ int s_rail[NT / 64], s_peak[NT / 64];
    const int tid = threadIdx.x;
    const size_t w = blockIdx.x;
    int rail = 0, peak = 0;
#pragma unroll 4
    for (int i = tid; i < N; i += NT) {
        const cpx v = pan_fetch<IQ, ALIGNED>(x, fmt, w * N + i);
        const float g = win[i];
        int hit = 0;
        pan_rail(v.x, fmt, hit, peak);
        if (IQ) pan_rail(v.y, fmt, hit, peak);
        rail += hit;
        s_re[i] = g * v.x; s_im[i] = g * v.y;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { rail += __shfl_xor(rail, d); const int o = __shfl_xor(peak, d); peak = o > peak ? o : peak; }
    if ((tid & 63) == 0) { s_rail[tid >> 6] = rail; s_peak[tid >> 6] = peak; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < NT / 64; k++) { rail += s_rail[k]; peak = s_peak[k] > peak ? s_peak[k] : peak; }
        wstat[2 * w] = rail; wstat[2 * w + 1] = peak;
    }
    pan_passes<N, N, 1, 5, 0, IQ>(s_re, s_im, tw, pw + w * BINS, tid);
}

// Row r0 + blockIdx.x of the launch, whose windows [w0, w0 + n_win) lie in pw / wstat; blockIdx.y < bins / 128: the bins
// 128 blockIdx.y + tid; blockIdx.y == bins / 128: the statistics.  ring [slots][bins], rstat [slots][2], row r at r mod slots.  A row
// whose first window is in this launch starts from zero, another one from what its slot holds.
__global__ __launch_bounds__(PAN_ROWS_NT) void k_pan_rows(const float* __restrict__ pw, const int32_t* __restrict__ wstat, long long w0, int n_win, long long A,
                                                          int bins, long long r0, float* __restrict__ ring, int32_t* __restrict__ rstat, long long slots) {
    __shared__ int s_c[PAN_ROWS_NT / 64], s_p[PAN_ROWS_NT / 64];
    const long long r = r0 + blockIdx.x, lo = r * A > w0 ? r * A : w0, hi = (r + 1) * A < w0 + n_win ? (r + 1) * A : w0 + n_win;
    if (lo >= hi) return;
    const bool fresh = lo == r * A;
    const size_t slot = (size_t)(r % slots);
    const int tid = threadIdx.x;
    if ((int)blockIdx.y < bins / PAN_ROWS_NT) {
        const int j = blockIdx.y * PAN_ROWS_NT + tid;
        float* dst = ring + slot * bins + j;
        const float* src = pw + (size_t)(lo - w0) * bins + j;
        float acc = fresh ? 0.0f : *dst;
        const int n = (int)(hi - lo);
        int i = 0;
        for (; i + 32 <= n; i += 32) {                                 // 32 loads in flight (a row has few threads and many windows: the
            float t[32];                                               // loop is bound by the loads' latency), added in window order
#pragma unroll
            for (int k = 0; k < 32; k++) t[k] = src[(size_t)(i + k) * bins];
#pragma unroll
            for (int k = 0; k < 32; k++) acc = acc + t[k];
        }
        for (; i < n; i++) acc = acc + src[(size_t)i * bins];
        *dst = acc;
    } else {
        int c = 0, p = 0;
        for (long long w = lo + tid; w < hi; w += PAN_ROWS_NT) { c += wstat[2 * (w - w0)]; const int q = wstat[2 * (w - w0) + 1]; p = q > p ? q : p; }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { c += __shfl_xor(c, d); const int o = __shfl_xor(p, d); p = o > p ? o : p; }
        if ((tid & 63) == 0) { s_c[tid >> 6] = c; s_p[tid >> 6] = p; }
        __syncthreads();
        if (tid == 0) {
            c = s_c[0] + s_c[1]; p = s_p[0] > s_p[1] ? s_p[0] : s_p[1];
            if (!fresh) { c += rstat[2 * slot]; p = rstat[2 * slot + 1] > p ? rstat[2 * slot + 1] : p; }
            rstat[2 * slot] = c; rstat[2 * slot + 1] = p;
        }
    }
}
