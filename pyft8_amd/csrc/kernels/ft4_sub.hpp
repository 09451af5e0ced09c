// ft4_sub.hpp -- FT4 signal subtraction (extension; ft8rx_ft4_subtract, ft8rx_ft4_sub_probe).  pyft8_amd/ft4.py
// holds the float64 twin that defines every step (sub_model, sub_bins, sub_refine, subtract).  Per decoded signal:
//   model    s[n], n < 60480 = 105 x 576: the complex form of the 4-GFSK transmit waveform (BT = 1.0, raised-cosine ramp symbols)
//   analysis y[n] = x[s0 + n] conj(s[n]), x = 0 outside the frame; A[k] = sum_n y[n] e^{-2 pi i k n / 60480}, k = -20 .. 20
//   refine   E(d) = sum_k |A_d[k]|^2 with the start at s0 + d, d = -24, -20 .. 24; the first maximum wins and is written back
//   apply    x[s0 + n] -= 2 Re(a[n] s[n]),  a[n] = (1 / 60480) sum_k A[k] e^{+2 pi i k n / 60480}
// on a float32 working copy of the frames; the signals of one frame go in list order, signal s of all rows at once:
//   k_ft4_sub_bins  (block, row, trial): the 41 bins of the block's 20 symbols at start + shift[trial] -> part[row][trial][block][41]
//   k_ft4_sub_pick  (row): E(d) = fixed-order sums of the partials; the first maximum -> best[row], the start written back
//   k_ft4_sub_apply (block, row): bins = fixed-order sum of the winning trial's partials; synthesis; the subtraction in place
//   k_ft4_sub_model (block, row): the model's samples (the stage entry)
// A symbol is 576 samples = 64 lanes x 9; a wavefront owns a run of FT4S_SPW whole symbols, a block four runs.  The phase of sample n:
// the carrier part is (fq n mod 4608) / 4608 of a turn, exact in integers (fq < 4608, n < 60480: the product stays below 2^29); the
// pulse part is, in fp64, the tones before the symbol plus three entries of the pulse's running sum (FT4S_PC), reduced to a fraction
// of a turn before it meets the carrier part.  Bins +k and -k share their phasor w^k = e^{-2 pi i k n / 60480} (w^-k is its
// conjugate), so a sample costs twenty rotations and four products per pair: per-lane sums in fp32 (45 terms), the cross-lane and
// cross-wave sums in fp64 in a fixed order.  No atomics: the residual is the same bytes on every run.
// Samples outside [0, 90000) are read as zero through a clamped address and a select, and are never written.
#ifndef FT8RX_FT4_SUB_HPP
#define FT8RX_FT4_SUB_HPP

#define FT4S_N (FT4_NSYM * FT4_NSPS)            /* 60480 */
#define FT4S_K 20                               /* bins -20 .. +20 */
#define FT4S_NB (2 * FT4S_K + 1)
#define FT4S_NT 13                              /* refine trials: shifts -24, -20 .. +24 samples */
#define FT4S_SPW 5                              /* symbols per wavefront run: 105 = 21 x 5 */
#define FT4S_RUNS (FT4_NSYM / FT4S_SPW)         /* 21 */
#define FT4S_GRIDX ((FT4S_RUNS + 3) / 4)        /* 6 blocks of four wavefronts */
#define FT4S_PC (3 * FT4_NSPS + 1)              /* exclusive running sum of the pulse: PC[j] = sum_{t < j} pulse[t], j = 0 .. 1728 */
static_assert(FT4S_RUNS * FT4S_SPW == FT4_NSYM && FT4_NSPS == 64 * 9, "a wavefront walks whole symbols, nine samples per lane");

struct Ft4SubShifts { int n; int shift[FT4S_NT]; };
// row r of a launch: signal s of sigs[r][max_sigs] where s < counts[r]; its audio is frame (frame_of ? frame_of[r] : r) of the working copy
struct Ft4SubSel { ft8rx_ft4_subsig* sigs; const int32_t* counts; const int32_t* frame_of; int max_sigs; int s; };
// LDS: the signal, ext[i] = the tone of symbol i - 1 with the two dummy edge symbols, and the pulse phase (in symbols' worth of
// pulse area, PC[1728] each) of everything before symbol q
struct Ft4SubModel { int start, fq; uint8_t ext[FT4_NSYM + 2 + 1]; double base[FT4_NSYM]; };

// The prologue of every per-signal kernel: false where the row has no signal s (block-uniform).  Every thread of the block calls.
FT8_DEV bool ft4s_begin(const Ft4SubSel& sel, int row, const double* __restrict__ pc, Ft4SubModel* M) {
    if (sel.s >= sel.counts[row]) return false;
    const ft8rx_ft4_subsig* g = sel.sigs + (size_t)row * sel.max_sigs + sel.s;
    const int tid = threadIdx.x;
    if (tid == 0) { M->start = g->start; M->fq = g->fq; }
    if (tid < FT4_NSYM + 2) { const int i = tid == 0 ? 0 : tid > FT4_NSYM ? FT4_NSYM - 1 : tid - 1; M->ext[tid] = g->tones[i] & 3; }
    __syncthreads();
    if (tid < FT4_NSYM) {
        // sum over the symbols i < q of ext[i] x (their whole pulse), less what of ext[0] and ext[1] lies before sample 0
        int a = 0;
        for (int i = 0; i < tid; i++) a += M->ext[i];
        M->base[tid] = (double)a * pc[FT4S_PC - 1] - ((double)M->ext[0] * pc[2 * FT4_NSPS] + (double)M->ext[1] * pc[FT4_NSPS]);
    }
    __syncthreads();
    return true;
}

// sample n = 576 q + r of the model: (sr, si) = amp e^{i phi[n]}
FT8_DEV void ft4s_signal(const Ft4SubModel& M, const double* __restrict__ pc, int q, int r, float* sr, float* si) {
    const double area = M.base[q] + ((double)M.ext[q] * pc[r + 2 * FT4_NSPS] + (double)M.ext[q + 1] * pc[r + FT4_NSPS] + (double)M.ext[q + 2] * pc[r]);
    const double turns = area * (1.0 / (double)FT4_NSPS);               // 20.8333 / 12000 of a turn per unit of pulse area
    const int cph = (M.fq * (FT4_NSPS * q + r)) % 4608;
    float fr = (float)(turns - floor(turns)) + (float)cph * (1.0f / 4608.0f);
    fr = fr >= 1.0f ? fr - 1.0f : fr;
    const float s = __builtin_amdgcn_sinf(fr), c = __builtin_amdgcn_cosf(fr);
    float amp = 1.0f;
    if (q == 0) amp = 0.5f * (1.0f - __builtin_amdgcn_cosf((float)r * (1.0f / 1152.0f)));
    else if (q == FT4_NSYM - 1) amp = 0.5f * (1.0f - __builtin_amdgcn_cosf((float)(FT4_NSPS - 1 - r) * (1.0f / 1152.0f)));
    *sr = amp * c; *si = amp * s;
}

// the symbols of this wavefront's run, every sample with the model's value: f(n, sr, si); nothing for a wavefront beyond the last run
template <class F> FT8_DEV void ft4s_walk(const Ft4SubModel& M, const double* __restrict__ pc, F f) {
    const int run = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (run >= FT4S_RUNS) return;
    for (int q = run * FT4S_SPW; q < (run + 1) * FT4S_SPW; q++) {
#pragma unroll 1
        for (int j = 0; j < 9; j++) {
            const int r = lane + 64 * j;
            float sr, si;
            ft4s_signal(M, pc, q, r, &sr, &si);
            f(FT4_NSPS * q + r, sr, si);
        }
    }
}
// w = e^{-2 pi i n / 60480}
FT8_DEV void ft4s_w(int n, float* wr, float* wi) {
    const float rv = (float)n * (1.0f / (float)FT4S_N);
    *wr = __builtin_amdgcn_cosf(rv); *wi = -__builtin_amdgcn_sinf(rv);
}
FT8_DEV float ft4s_sample(const float* __restrict__ x, int idx) {
    const int ic = idx < 0 ? 0 : idx > FT8RX_FT4_NSAMP - 1 ? FT8RX_FT4_NSAMP - 1 : idx;
    const float v = x[ic];
    return (idx >= 0 && idx < FT8RX_FT4_NSAMP) ? v : 0.0f;
}

// part [rows][FT4S_NT][FT4S_GRIDX][FT4S_NB]: index k + 20 holds bin k
__global__ __launch_bounds__(256) void k_ft4_sub_bins(const float* __restrict__ wf, Ft4SubSel sel, const double* __restrict__ pc, Ft4SubShifts sh,
                                                      double2* __restrict__ part) {
    __shared__ Ft4SubModel M;
    __shared__ double2 red[4][FT4S_NB];
    const int row = blockIdx.y, trial = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (!ft4s_begin(sel, row, pc, &M)) return;
    const float* x = wf + (size_t)(sel.frame_of ? sel.frame_of[row] : row) * FT8RX_FT4_NSAMP;
    const int s0 = M.start + sh.shift[trial];
    // y r and y conj(r) share the four products yr rr, yi ri, yr ri, yi rr: their sums per pair of bins
    float p1[FT4S_K], p2[FT4S_K], p3[FT4S_K], p4[FT4S_K], zr = 0.0f, zi = 0.0f;
#pragma unroll
    for (int k = 0; k < FT4S_K; k++) { p1[k] = 0.0f; p2[k] = 0.0f; p3[k] = 0.0f; p4[k] = 0.0f; }
    ft4s_walk(M, pc, [&](int n, float sr, float si) {
        const float xv = ft4s_sample(x, s0 + n);
        const float yr = xv * sr, yi = -(xv * si);                    // y = x conj(s)
        float wr, wi;
        ft4s_w(n, &wr, &wi);
        zr += yr; zi += yi;
        float rr = wr, ri = wi;
#pragma unroll
        for (int k = 0; k < FT4S_K; k++) {
            p1[k] += yr * rr; p2[k] += yi * ri; p3[k] += yr * ri; p4[k] += yi * rr;
            const float t = rr * wr - ri * wi; ri = rr * wi + ri * wr; rr = t;
        }
    });
    {
        double vr = (double)zr, vi = (double)zi;
        wave_sum2(vr, vi);
        if (lane == 0) red[wave][FT4S_K] = make_double2(vr, vi);
    }
#pragma unroll
    for (int k = 0; k < FT4S_K; k++) {
        double ar = (double)p1[k] - (double)p2[k], ai = (double)p3[k] + (double)p4[k];        // bin +(k + 1): y w^(k + 1)
        double br = (double)p1[k] + (double)p2[k], bi = (double)p4[k] - (double)p3[k];        // bin -(k + 1): y conj(w^(k + 1))
        wave_sum2(ar, ai); wave_sum2(br, bi);
        if (lane == 0) { red[wave][FT4S_K + 1 + k] = make_double2(ar, ai); red[wave][FT4S_K - 1 - k] = make_double2(br, bi); }
    }
    __syncthreads();
    if (tid < FT4S_NB) {
        const double2 a = red[0][tid], b = red[1][tid], c = red[2][tid], d = red[3][tid];
        part[(((size_t)row * FT4S_NT + trial) * FT4S_GRIDX + blockIdx.x) * FT4S_NB + tid] = make_double2((a.x + b.x) + (c.x + d.x), (a.y + b.y) + (c.y + d.y));
    }
}

// bin tid - 20 of (row, trial): the partials in block order
FT8_DEV double2 ft4s_bin(const double2* __restrict__ part, int row, int trial, int b) {
    const double2* p = part + ((size_t)row * FT4S_NT + trial) * FT4S_GRIDX * FT4S_NB + b;
    double vr = 0.0, vi = 0.0;
    for (int c = 0; c < FT4S_GRIDX; c++) { vr += p[c * FT4S_NB].x; vi += p[c * FT4S_NB].y; }
    return make_double2(vr, vi);
}

// one wavefront per row: E(d) of the sh.n trials, the first maximum -> best[row]; the start moves there.  energy (optional) [rows][FT4S_NT]
__global__ __launch_bounds__(64) void k_ft4_sub_pick(Ft4SubSel sel, Ft4SubShifts sh, const double2* __restrict__ part, int32_t* __restrict__ best,
                                                     double* __restrict__ energy) {
    const int row = blockIdx.x, lane = threadIdx.x;
    if (sel.s >= sel.counts[row]) return;
    double be = 0.0; int bi = 0;
    for (int t = 0; t < sh.n; t++) {
        double e = 0.0, unused = 0.0;
        if (lane < FT4S_NB) { const double2 a = ft4s_bin(part, row, t, lane); e = a.x * a.x + a.y * a.y; }
        wave_sum2(e, unused);
        if (t == 0 || e > be) { be = e; bi = t; }
        if (energy && lane == 0) energy[(size_t)row * FT4S_NT + t] = e;
    }
    if (lane == 0) {
        best[row] = bi;
        sel.sigs[(size_t)row * sel.max_sigs + sel.s].start += sh.shift[bi];
    }
}

// wf -= the signal at its (refined) start, from the bins of trial best[row] (whose shift the start already holds)
__global__ __launch_bounds__(256) void k_ft4_sub_apply(float* __restrict__ wf, Ft4SubSel sel, const double* __restrict__ pc, const double2* __restrict__ part,
                                                       const int32_t* __restrict__ best) {
    __shared__ Ft4SubModel M;
    __shared__ float Ar[FT4S_NB], Ai[FT4S_NB];
    const int row = blockIdx.y, tid = threadIdx.x;
    if (!ft4s_begin(sel, row, pc, &M)) return;
    if (tid < FT4S_NB) {
        const double2 a = ft4s_bin(part, row, best[row], tid);
        Ar[tid] = (float)(a.x / (double)FT4S_N); Ai[tid] = (float)(a.y / (double)FT4S_N);
    }
    __syncthreads();
    float* x = wf + (size_t)(sel.frame_of ? sel.frame_of[row] : row) * FT8RX_FT4_NSAMP;
    const int s0 = M.start;
    ft4s_walk(M, pc, [&](int n, float sr, float si) {
        float wr, wi;
        ft4s_w(n, &wr, &wi);
        wi = -wi;                                                     // e^{+2 pi i n / 60480}
        float er = Ar[FT4S_K], ei = Ai[FT4S_K], rr = wr, ri = wi;
#pragma unroll
        for (int k = 1; k <= FT4S_K; k++) {
            const float ar = Ar[FT4S_K + k], ai = Ai[FT4S_K + k], br = Ar[FT4S_K - k], bi = Ai[FT4S_K - k];
            er += (ar * rr - ai * ri) + (br * rr + bi * ri);          // A[k] r + A[-k] conj(r)
            ei += (ar * ri + ai * rr) + (bi * rr - br * ri);
            const float t = rr * wr - ri * wi; ri = rr * wi + ri * wr; rr = t;
        }
        const int g = s0 + n;
        if (g >= 0 && g < FT8RX_FT4_NSAMP) x[g] = x[g] - 2.0f * (er * sr - ei * si);
    });
}

// the stage entry's model: model [rows][60480] (re, im)
__global__ __launch_bounds__(256) void k_ft4_sub_model(Ft4SubSel sel, const double* __restrict__ pc, float2* __restrict__ model) {
    __shared__ Ft4SubModel M;
    const int row = blockIdx.y;
    if (!ft4s_begin(sel, row, pc, &M)) return;
    float2* o = model + (size_t)row * FT4S_N;
    ft4s_walk(M, pc, [&](int n, float sr, float si) { o[n] = make_float2(sr, si); });
}

#endif
