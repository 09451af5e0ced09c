// ddc_rat_ring.hpp -- what is the rational resampler's own in its index arithmetic (ft8rx_ddc_rat*): the plan of a
// rate, the limits, the inputs an intermediate sample reads, the history the stream keeps, how many outputs a tile of either kernel
// regime holds.  Which intermediate samples a push completes, the origin and the history ring are ddc_pre_ring.hpp's.  Pure functions
// of 64-bit indices.  No HIP: compiles with plain g++ (tests/ddc_rat_ring_check.cpp checks it under the host sanitizers).
//
// Indices are ABSOLUTE: input sample n counts from index 0 of the sample clock; intermediate sample k sits at input time k M / L, with
// rate_mid = rate L / M.  With the prototype h of N taps (odd), C = (N - 1) / 2 and t_k = k M + C,
//   v[k] = g0 sum_{j = t_k (mod L)} h[j] u[(t_k - j) / L]  =  g0 sum_{i < P} h[phi_k + i L] u[b_k - i],   b_k = t_k / L,  phi_k = t_k mod L,
// P = ceil(N / L) taps per phase (h is zero from N on): the last input of k is b_k, the first one b_k - P + 1 or later.  n < 2^52 and
// L <= 320, so every product fits 64 bits.  The stream begins at n_origin, where k_origin = n_origin L / M is an integer on the tile grid
// of the stage behind (a multiple of 1008 rate_mid / 12000), and the input is zero before it.
#pragma once
#include <cstdint>

#include "ddc_wide_ring.hpp"

namespace ddcrat {

constexpr int64_t RATE_MIN = 16000, RATE_MAX = 129600000;
constexpr int64_t MAX_L = 320;                       // largest interpolation factor (22050 Hz: 320 / 147)
constexpr int64_t MAX_TAPS = ddcwide::MAX_TAPS;      // bound of len(h): the wide path's table bound
constexpr int64_t N_MAX = (int64_t)1 << 52;          // bound of an origin; a stream ends below 2 N_MAX, so that n L stays below 2^62

constexpr int64_t gcd(int64_t a, int64_t b) { return b ? gcd(b, a % b) : a; }

// rate_mid = the one of 192000, 96000, 48000 with the smallest L = mid / gcd(rate, mid), ties to the largest; M = rate / gcd.
// rate_mid = 0: refused -- outside [RATE_MIN, RATE_MAX], a rate the plain down-converter (12000 x 1, 2, 4, 8, 16) or the wide
// pre-decimator takes, or L > MAX_L.  (The filter length is the other limit: ft8rx_ddc_rat_plan.)
struct Plan { int64_t rate_mid, L, M; };
constexpr Plan plan(int64_t rate) {
    if (rate < RATE_MIN || rate > RATE_MAX) return Plan{0, 0, 0};
    for (int64_t d = 1; d <= 16; d *= 2) if (rate == 12000 * d) return Plan{0, 0, 0};
    if (ddcwide::plan(rate).rate_mid) return Plan{0, 0, 0};
    Plan best{0, 0, 0};
    for (int64_t mid = 192000; mid >= 48000; mid /= 2) {
        const int64_t g = gcd(rate, mid);
        if (!best.rate_mid || mid / g < best.L) best = Plan{mid, mid / g, rate / g};
    }
    return best.L <= MAX_L ? best : Plan{0, 0, 0};
}

constexpr int64_t phase_taps(int64_t N, int64_t L) { return (N + L - 1) / L; }      // P

// the last input of intermediate sample k, its phase, and the first input the kernel reads for it (P table entries, zero-padded)
inline int64_t last_input(int64_t k, int64_t N, int64_t L, int64_t M) { return (k * M + (N - 1) / 2) / L; }
inline int64_t phase(int64_t k, int64_t N, int64_t L, int64_t M) { return (k * M + (N - 1) / 2) % L; }
inline int64_t first_input(int64_t k, int64_t N, int64_t L, int64_t M) { return last_input(k, N, L, M) - phase_taps(N, L) + 1; }

// The kernel's two regimes (kernels/ddc_rat.hpp), chosen by the plan alone.
// LANE: one lane per output; the channel's table [L][P] (at most LANE_TABLE entries) and the tile's input span (at most LANE_SAMPLES)
// are in LDS.  WAVE: a wave per output as in the wide kernel; the taps go by in pieces of PIECE over an LDS image of WAVE_SAMPLES.
constexpr int64_t LANE_P = 64, LANE_TABLE = 3072, LANE_SAMPLES = 3200, LANE_TILE = 256;
constexpr int64_t PIECE = 1024, WAVE_SAMPLES = 6144, WAVE_TILE = 16;
constexpr bool lane_regime(int64_t N, int64_t L) { return phase_taps(N, L) <= LANE_P && phase_taps(N, L) * L <= LANE_TABLE; }
// outputs per tile: consecutive outputs k0 .. k0 + t - 1 end at inputs that span at most (t - 1) M / L + 1, and each reads `taps` back
constexpr int64_t tile_fit(int64_t samples, int64_t taps, int64_t L, int64_t M, int64_t most) {
    const int64_t t = (samples - taps - 1) * L / M + 1;
    return t < most ? t : most;
}
constexpr int64_t tile_outputs(int64_t N, int64_t L, int64_t M) {
    return lane_regime(N, L) ? tile_fit(LANE_SAMPLES, phase_taps(N, L), L, M, LANE_TILE) : tile_fit(WAVE_SAMPLES, PIECE, L, M, WAVE_TILE);
}

// samples of history the stream keeps: an intermediate sample that is not complete ends at the newest input or later, and reads
// less than P back from there
constexpr int64_t history(int64_t N, int64_t L) { return phase_taps(N, L); }

// the shared arithmetic under this stage's names, the origin with this stage's bound
inline bool origin_ok(int64_t n_origin, int64_t rate_mid, int64_t L, int64_t M) { return ddcpre::origin_ok(n_origin, N_MAX, rate_mid, L, M); }
using ddcpre::k_origin;
using ddcpre::mid_done;
using ddcpre::mid_count;
using ddcpre::hist_pos;
using ddcpre::Keep;
using ddcpre::keep;

}  // namespace ddcrat
