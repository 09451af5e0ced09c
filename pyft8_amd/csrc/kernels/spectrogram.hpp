// spectrogram.hpp -- K1: 375-hop dB spectrogram (receiver.py:288-306)
// Part of libft8rx.so.  The arithmetic of a row, spectrogram_hop, is shared device code of both translation units; k_spectrogram /
// k_hop_spectrum are built in the second one only (ft8rx_ilp.hip, ILP scheduling: FT8RX_ILP_UNIT) and launched through ilp_launch.hpp;
// k_fill_row0, k_grid_stream (rows off the streaming down-converter's output ring) and k_spectrogram_f32 (float32
// frames) belong to the main unit.
#ifndef FT8RX_SPECTROGRAM_HPP
#define FT8RX_SPECTROGRAM_HPP

// ------------------------------------------------------------------------------------ K1 spectrogram
// one hop: window samples a[base .. base+3840) (zeros before the frame start) -> 976 dB values.
// 128 threads; 1920-point complex FFT (plan [8,4,4,5,3]) in place in one LDS image as three register-fused stages:
//   [8]    240 butterflies straight from global memory (int16 -> f32, Hann window fused in),
//   [4,4]  120 groups of 16 (one per thread), twiddles from the LDS table w240[t] = W1920[8 t],
//   [5,3]  128 groups of 15 (one per thread), compile-time twiddles,
// then the real-FFT split and 20 log10|.|.
// Where the samples come from is the caller's: load(m) -> samples 2 m (.x) and 2 m + 1 (.y) of the window as floats, m = 0 .. 1919
// (SpecLoadFrame / SpecLoadFrameF32: an int16 / float32 frame in memory; SpecLoadRing / SpecLoadRingF32: the down-converter's output
// rings).  The int16 loaders convert exactly, (float)(int16_t); the float32 ones hand the samples on as they are.
#define SPEC_NT 128
// a[base .. base + 3840) of an int16 array, base even: one aligned pair per load; zeros where the index is negative
struct SpecLoadFrame {
    const int16_t* __restrict__ a; int base;
    FT8_DEV float2 operator()(int m) const {
        const int i0 = base + 2 * m;
        // samples before the frame start are zeros (the ring starts zeroed, receiver.py:248): masked with integer ALU ops --
        // a select here is turned back into a branch around the load, i.e. one memory round trip per basic block
        uint32_t raw = *reinterpret_cast<const uint32_t*>(a + (i0 & ~(i0 >> 31)));
        raw &= ~(uint32_t)(i0 >> 31);
        return make_float2((float)(int16_t)(raw & 0xFFFFu), (float)(int16_t)(raw >> 16));
    }
};
// the same window of a float32 array (8-byte aligned, base even): one aligned 8-byte load per pair from the clamped address, zeros
// before the frame start by masking the bit patterns
struct SpecLoadFrameF32 {
    const float* __restrict__ a; int base;
    FT8_DEV float2 operator()(int m) const {
        const int i0 = base + 2 * m;
        const uint32_t keep = ~(uint32_t)(i0 >> 31);
        const uint2 raw = *reinterpret_cast<const uint2*>(a + (i0 & (int)keep));
        return make_float2(__uint_as_float(raw.x & keep), __uint_as_float(raw.y & keep));
    }
};

template <class Load>
FT8_DEV void spectrogram_hop(const Load& load, float* __restrict__ out, const Tables& T, cpx* z, cpx* w240, int tid) {
    const cpx* __restrict__ W = T.W1920;
    // stage-2 twiddle table: requested now, stored to LDS just before the first barrier (a load -> wait -> store loop here delayed
    // the whole block by a memory round trip before its first sample load)
    const cpx wa = W[8 * tid], wb = W[8 * (tid + SPEC_NT < 240 ? tid + SPEC_NT : 0)];
    {   // pass [8]: n = 1920, s = 1, m = 240: butterfly p reads samples m = p + 240 j.  Straight-line: loads from clamped addresses,
        // zeros by masking (hops before the frame start: the loads above), twiddle multiplies unconditional (W^0 = (1, -0) is an exact identity).
        cpx v[2][8];
        cpx w[2][8];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int p = tid + SPEC_NT * i;
            const int pc = (p < 240) ? p : 239;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int m = pc + 240 * j;
                const float2 x = load(m);
                const float2 wn = *reinterpret_cast<const float2*>(T.win + 2 * m);
                v[i][j] = make_float2(x.x * wn.x, x.y * wn.y);
            }
#pragma unroll
            for (int j = 1; j < 8; j++) w[i][j] = W[j * pc];
        }
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int p = tid + SPEC_NT * i;
            dft<8>(v[i]);
#pragma unroll
            for (int j = 1; j < 8; j++) v[i][j] = cmul(v[i][j], w[i][j]);
            if (p < 240) {
#pragma unroll
                for (int j = 0; j < 8; j++) z[8 * p + j] = v[i][j];
            }
        }
    }
    w240[tid] = wa;
    if (tid + SPEC_NT < 240) w240[tid + SPEC_NT] = wb;
    __syncthreads();
    {   // passes [4,4]: n = 240, s = 8; group g = (pp = g / 8, q = g % 8): in q + 8(pp + 15 j' + 60 j), out q + 8 j + 32(4 pp + j')
        typedef Fused2<1920, 240, 8, 4, 4> F;
        cpx v[4][4];
        const bool on = tid < F::groups;
        if (on) F::load_affine<120, 480>(z, tid, v);
        __syncthreads();
        if (on) {
            const int pp = tid >> 3;
#pragma unroll
            for (int jp = 0; jp < 4; jp++) {
                dft<4>(v[jp]);
                const int pq = pp + 15 * jp;
#pragma unroll
                for (int j = 1; j < 4; j++) v[jp][j] = cmul(v[jp][j], w240[j * pq]);          // W1920[j p 8]
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                cpx u[4];
#pragma unroll
                for (int jp = 0; jp < 4; jp++) u[jp] = v[jp][j];
                dft<4>(u);
#pragma unroll
                for (int jp = 1; jp < 4; jp++) u[jp] = cmul(u[jp], w240[4 * jp * pp]);        // W1920[j' pp 32]
#pragma unroll
                for (int jp = 0; jp < 4; jp++) v[jp][j] = u[jp];
            }
            F::store_affine<32, 8>(z, (tid & 7) + 128 * (tid >> 3), v);
        }
        __syncthreads();
    }
    {   // passes [5,3]: n = 15, s = 128; group q: in q + 128 (j' + 3 j), out q + 128 j + 640 j'
        typedef Fused2<1920, 15, 128, 5, 3> F;
        cpx v[3][5];
        F::load_affine<128, 384>(z, tid, v);
        __syncthreads();
        F::compute_pp(0, v, W);
        F::store_affine<640, 128>(z, tid, v);
        __syncthreads();
    }
    // real-FFT split + dB: the split twiddles of the thread's eight bins are requested together, ahead of the sqrt/log10 chain
    // (with the load inside the loop every iteration waited for its own twiddle: 498 -> 467 us)
    constexpr int NE = (FT8RX_GRID_COLS + SPEC_NT - 1) / SPEC_NT;
    cpx we[NE];
#pragma unroll
    for (int q = 0; q < NE; q++) { const int k = tid + SPEC_NT * q; we[q] = T.WR3840[k < FT8RX_GRID_COLS ? k : 0]; }
#pragma unroll
    for (int q = 0; q < NE; q++) {
        const int k = tid + SPEC_NT * q;
        if (k >= FT8RX_GRID_COLS) break;
        cpx p = z[k], q2 = z[(1920 - k) % 1920];
        float er = 0.5f * (p.x + q2.x), ei = 0.5f * (p.y - q2.y);
        float orr = 0.5f * (p.y + q2.y), oi = 0.5f * (q2.x - p.x);
        cpx w = we[q];
        float xr = er + (w.x * orr - w.y * oi);
        float xi = ei + (w.x * oi + w.y * orr);
        // 20 log10(|X| + 1e-12) (receiver.py:292) as 10 log10(max(|X|^2, 1e-24)) -- the contract's form: the same value to far below a
        // float ulp for any |X| > 1e-6, exactly -240 dB for |X| = 0, and no IEEE square root (a dozen instructions) per bin
        float pw = xr * xr + xi * xi;
        pw = (pw > 1e-24f) ? pw : 1e-24f;
        out[k] = 10.0f * ft8_log10f_normal(pw);                  // 1e-24 <= argument, normal; finite inside the domain of float frames
    }
}

#ifdef FT8RX_ILP_UNIT
__global__ __launch_bounds__(SPEC_NT) void k_spectrogram(const int16_t* __restrict__ audio, float* __restrict__ grid, Tables T) {
    __shared__ cpx z[1920];
    __shared__ cpx w240[240];
    // XCD-aware hop mapping: workgroup id -> XCD is id % 8 and gridDim.x = 376 = 8 * 47, so the 47 workgroups of a
    // frame that land on one XCD take 47 consecutive hops: each XCD's L2 then sees one eighth of the frame's audio
    // (8x overlapping windows) instead of all of it.
    static_assert(FT8RX_GRID_ROWS == 8 * 47, "the hop map below assumes gridDim.x = 376 = 8 XCDs x 47");
    const int hop = (blockIdx.x & 7) * 47 + (blockIdx.x >> 3) + 1, f = blockIdx.y, tid = threadIdx.x;
    if (hop > 375) {           // the one spare workgroup of a frame: the never-written row 0 (receiver.py:240), which the cycle FFT's scratch overwrites
        float* row0 = grid + (size_t)f * FT8RX_GRID_ROWS * FT8RX_GRID_COLS;
        for (int i = tid; i < FT8RX_GRID_COLS; i += SPEC_NT) row0[i] = 1.0f;
        return;
    }
    spectrogram_hop(SpecLoadFrame{audio + (size_t)f * FT8RX_NSAMP, 480 * hop - 3840},
                    grid + ((size_t)f * FT8RX_GRID_ROWS + hop) * FT8RX_GRID_COLS, T, z, w240, tid);
}

// streaming mode: one hop of the live receiver (AudioIn.get_hop_spectrum, receiver.py:288-293)
__global__ __launch_bounds__(SPEC_NT) void k_hop_spectrum(const int16_t* __restrict__ win3840, float* __restrict__ row, Tables T) {
    __shared__ cpx z[1920];
    __shared__ cpx w240[240];
    spectrogram_hop(SpecLoadFrame{win3840, 0}, row, T, z, w240, threadIdx.x);
}

#else
__global__ void k_fill_row0(float* grid, int B) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * FT8RX_GRID_COLS) grid[(size_t)(i / FT8RX_GRID_COLS) * FT8RX_GRID_ROWS * FT8RX_GRID_COLS + (i % FT8RX_GRID_COLS)] = 1.0f;
}

// k_spectrogram on float32 frames: the same XCD hop map, LDS layout and row-0 workgroup; audio 8-byte aligned
__global__ __launch_bounds__(SPEC_NT) void k_spectrogram_f32(const float* __restrict__ audio, float* __restrict__ grid, Tables T) {
    __shared__ cpx z[1920];
    __shared__ cpx w240[240];
    static_assert(FT8RX_GRID_ROWS == 8 * 47, "the hop map below assumes gridDim.x = 376 = 8 XCDs x 47");
    const int hop = (blockIdx.x & 7) * 47 + (blockIdx.x >> 3) + 1, f = blockIdx.y, tid = threadIdx.x;
    if (hop > 375) {
        float* row0 = grid + (size_t)f * FT8RX_GRID_ROWS * FT8RX_GRID_COLS;
        for (int i = tid; i < FT8RX_GRID_COLS; i += SPEC_NT) row0[i] = 1.0f;
        return;
    }
    spectrogram_hop(SpecLoadFrameF32{audio + (size_t)f * FT8RX_NSAMP, 480 * hop - 3840},
                    grid + ((size_t)f * FT8RX_GRID_ROWS + hop) * FT8RX_GRID_COLS, T, z, w240, tid);
}

// ------------------------------------------------------------------------------------ rows off the down-converter's output ring
// (index arithmetic: ddc_grid_ring.hpp).  A window of one channel's int16 output ring [ring_n]: sample i sits
// at slot + i, less ring_n once past the ring's end (one wrap at the most: slot < ring_n, i < 3840 <= ring_n); the first nz samples
// lie before the stream's origin and are zeros.  The first index may be odd, so the two samples of a pair are loaded one by one.
struct SpecLoadRing {
    typedef int16_t sample;
    const int16_t* __restrict__ ring; int slot, nz, ring_n;
    FT8_DEV float2 operator()(int m) const {
        int i0 = slot + 2 * m, i1 = i0 + 1;
        i0 -= (i0 >= ring_n) ? ring_n : 0;
        i1 -= (i1 >= ring_n) ? ring_n : 0;
        // zeros before the origin by masking, as SpecLoadFrame does (the addresses are inside the ring whatever nz is)
        const uint32_t lo = (uint32_t)(uint16_t)ring[i0] & ~(uint32_t)((2 * m - nz) >> 31);
        const uint32_t hi = (uint32_t)(uint16_t)ring[i1] & ~(uint32_t)((2 * m + 1 - nz) >> 31);
        return make_float2((float)(int16_t)lo, (float)(int16_t)hi);
    }
};
// the same window of one channel's float32 output ring (the stream runs float frames): the same wrap, the zeros by masking the bit patterns
struct SpecLoadRingF32 {
    typedef float sample;
    const float* __restrict__ ring; int slot, nz, ring_n;
    FT8_DEV float2 operator()(int m) const {
        int i0 = slot + 2 * m, i1 = i0 + 1;
        i0 -= (i0 >= ring_n) ? ring_n : 0;
        i1 -= (i1 >= ring_n) ? ring_n : 0;
        const uint32_t lo = __float_as_uint(ring[i0]) & ~(uint32_t)((2 * m - nz) >> 31);
        const uint32_t hi = __float_as_uint(ring[i1]) & ~(uint32_t)((2 * m + 1 - nz) >> 31);
        return make_float2(__uint_as_float(lo), __uint_as_float(hi));
    }
};

// one block per (new hop, channel): block (b, j) computes hop q_first + b of channel j from d_out [n_out][ring_n] into row
// (row0 + b) mod n_rows of d_grid [n_out][n_rows][FT8RX_GRID_COLS].  The host hands over the FIRST hop's ring slot (slot0 < ring_n),
// zero prefix (nz0 in [0, 3840)) and grid row (row0 < n_rows); hop b is 480 b samples on, and gridDim.x <= n_rows and
// 480 gridDim.x <= ring_n keep every wrap a single compare and subtract (ft8rx.hip: ddc_stream_push).
// Load: SpecLoadRing on the int16 ring, SpecLoadRingF32 on the float32 ring.
template <class Load>
__global__ __launch_bounds__(SPEC_NT) void k_grid_stream(const typename Load::sample* __restrict__ d_out, int ring_n, int slot0, int nz0,
                                                         float* __restrict__ d_grid, int n_rows, int row0, Tables T) {
    __shared__ cpx z[1920];
    __shared__ cpx w240[240];
    const int b = blockIdx.x, j = blockIdx.y;
    int slot = slot0 + 480 * b, row = row0 + b, nz = nz0 - 480 * b;
    slot -= (slot >= ring_n) ? ring_n : 0;
    row -= (row >= n_rows) ? n_rows : 0;
    nz = nz > 0 ? nz : 0;
    spectrogram_hop(Load{d_out + (size_t)j * ring_n, slot, nz, ring_n},
                    d_grid + ((size_t)j * n_rows + row) * FT8RX_GRID_COLS, T, z, w240, threadIdx.x);
}
#endif  // FT8RX_ILP_UNIT

#endif
