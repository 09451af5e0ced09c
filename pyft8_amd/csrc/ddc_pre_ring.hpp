// ddc_pre_ring.hpp -- the index arithmetic both input pre-stages share: the wide pre-decimator
// (ddc_wide_ring.hpp, section 16.2) and the rational resampler (ddc_rat_ring.hpp, section 16.3).  Which intermediate samples a push
// completes, the stream's origin, where a chunk lands in the history ring.  Pure functions of 64-bit indices.  No HIP: compiles with
// plain g++ (tests/ddc_wide_ring_check.cpp and tests/ddc_rat_ring_check.cpp check it under the host sanitizers).
//
// Indices are ABSOLUTE: input sample n counts from index 0 of the sample clock; intermediate sample k sits at input time k M / L, with
// rate_mid = rate L / M.  With a prototype of N taps (odd) and C = (N - 1) / 2, the last input of k is (k M + C) / L.  The wide stage
// is the case L = 1, M = R0: k = n / R0, last input k R0 + C0.  n L stays below 2^62 (the bound of an origin is the stage's own).
#pragma once
#include <cstdint>

namespace ddcpre {

// the intermediate sample of an origin, and whether n_origin is one: k_origin = n_origin L / M is an integer on the tile grid of the
// stage behind (a multiple of 1008 rate_mid / 12000), 0 <= n_origin <= n_max.  At L = 1 that is n_origin % (1008 rate / 12000) == 0,
// the wide stream's rule: rate = R0 rate_mid (tests/ddc_wide_ring_check.cpp holds the two to each other).
inline int64_t k_origin(int64_t n_origin, int64_t L, int64_t M) { return n_origin * L / M; }
inline bool origin_ok(int64_t n_origin, int64_t n_max, int64_t rate_mid, int64_t L, int64_t M) {
    if (n_origin < 0 || n_origin > n_max || (n_origin * L) % M != 0) return false;
    return (n_origin * L / M) % (1008 * (rate_mid / 12000)) == 0;
}

// absolute index of the first intermediate sample that is NOT complete when the inputs [.., n_end) exist: k is complete iff its last
// input, (k M + C) / L, is below n_end, i.e. k M + C < n_end L.  Never below the origin's sample.
inline int64_t mid_done(int64_t n_origin, int64_t n_end, int64_t N, int64_t L, int64_t M) {
    const int64_t k0 = k_origin(n_origin, L, M), have = n_end * L - (N - 1) / 2 - 1;
    if (have < 0) return k0;
    const int64_t k = have / M + 1;
    return k > k0 ? k : k0;
}

// intermediate samples of a one-shot call on n_samples inputs (zero outside): those whose first tap, h[0] at input (k M + C - N + 1) / L,
// can still meet a non-zero input, k M + C - (N - 1) <= (n_samples - 1) L; at most `cap` (15 s at the intermediate rate), at least one
inline int64_t mid_count(int64_t n_samples, int64_t N, int64_t L, int64_t M, int64_t cap) {
    if (n_samples < 1) return 1;
    const int64_t k = ((n_samples - 1) * L + (N - 1) / 2) / M + 1;
    return k < cap ? k : cap;
}

// position of absolute input n in the history ring of H samples (n >= n_origin)
inline int64_t hist_pos(int64_t n, int64_t n_origin, int64_t H) { return (n - n_origin) % H; }

// after a push of n_new samples, `pushed` samples having come before it: the chunk's last min(n_new, H) samples go into the ring, the
// first `skip` of the chunk are left out; `first` samples at pos up to the ring's end, `second` from its start
struct Keep { int64_t skip, pos, first, second; };
inline Keep keep(int64_t pushed, int64_t n_new, int64_t H) {
    const int64_t skip = n_new > H ? n_new - H : 0, n = n_new - skip;
    const int64_t pos = (pushed + skip) % H, room = H - pos;
    return Keep{skip, pos, n < room ? n : room, n < room ? 0 : n - room};
}

}  // namespace ddcpre
