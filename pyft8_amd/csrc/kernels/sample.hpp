// The one loader of the input stages (kernels/ddc.hpp, ddc_wide.hpp, ddc_rat.hpp): sample i of an array of format `fmt` (sample_fmt.hpp)
// as a float (real formats) or a complex float (IQ formats), the 8-bit formats on the int16 scale, exact in float32.  The format is a
// kernel argument, uniform over the launch: every test of it is a wave-uniform branch.
#pragma once

template <bool IQ> struct Sample;
template <> struct Sample<false> {
    typedef float T;
    static __device__ __forceinline__ float zero() { return 0.0f; }
    static __device__ __forceinline__ float fetch(const void* __restrict__ in, int fmt, size_t i) {
        return fmt == SF_REAL_I16 ? (float)((const int16_t*)in)[i] : ((const float*)in)[i];
    }
    static __device__ __forceinline__ void mac(float2 W, float x, float& ar, float& ai) { ar = fmaf(W.x, x, ar); ai = fmaf(W.y, x, ai); }
};
template <> struct Sample<true> {
    typedef float2 T;
    static __device__ __forceinline__ float2 zero() { return make_float2(0.0f, 0.0f); }
    static __device__ __forceinline__ float2 fetch(const void* __restrict__ in, int fmt, size_t i) {
        if (fmt == SF_IQ_I16) { const short2 v = ((const short2*)in)[i]; return make_float2((float)v.x, (float)v.y); }
        if (fmt == SF_IQ_F32) return ((const float2*)in)[i];
        if (fmt == SF_IQ_U8) { const uchar2 v = ((const uchar2*)in)[i]; return make_float2((float)(256 * (int)v.x - 32640), (float)(256 * (int)v.y - 32640)); }
        const char2 v = ((const char2*)in)[i];
        return make_float2((float)(256 * (int)v.x), (float)(256 * (int)v.y));
    }
    static __device__ __forceinline__ void mac(float2 W, float2 x, float& ar, float& ai) {
        ar = fmaf(W.x, x.x, ar); ar = fmaf(-W.y, x.y, ar);
        ai = fmaf(W.x, x.y, ai); ai = fmaf(W.y, x.x, ai);
    }
};

// sample n of one call's array: zero outside [0, n_samples)
template <bool IQ> struct ArrayLoad {
    const void* __restrict__ in; int fmt; long long n_samples;
    __device__ __forceinline__ typename Sample<IQ>::T operator()(long long n) const {
        return n < 0 || n >= n_samples ? Sample<IQ>::zero() : Sample<IQ>::fetch(in, fmt, (size_t)n);
    }
};
// sample n of a stream: zero outside [n_origin, n_end); [n_start, n_end) is the chunk of this push; what came before it is in the
// history ring of H samples (sample n_start - 1 at p_last, older ones before it, wrapping), of which a tile reaches back less than H
template <bool IQ> struct StreamLoad {
    const void* __restrict__ hist; int H, p_last; const void* __restrict__ chunk; int fmt; long long n_origin, n_start, n_end;
    __device__ __forceinline__ typename Sample<IQ>::T operator()(long long n) const {
        if (n < n_origin || n >= n_end) return Sample<IQ>::zero();
        if (n >= n_start) return Sample<IQ>::fetch(chunk, fmt, (size_t)(n - n_start));
        const long long d = n_start - 1 - n;
        if (d >= H) return Sample<IQ>::zero();          // (no complete output reaches that far back)
        const int p = p_last - (int)d;
        return Sample<IQ>::fetch(hist, fmt, (size_t)(p < 0 ? p + H : p));
    }
};
