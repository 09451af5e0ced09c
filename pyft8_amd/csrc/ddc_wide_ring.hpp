// ddc_wide_ring.hpp -- what is the wide pre-decimator's own in its index arithmetic (ft8rx_ddc_wide*): the plan
// of a rate, the limits, the history the stream keeps, how many outputs a tile of the kernel holds.  Which intermediate samples a push
// completes, the origin and the history ring are ddc_pre_ring.hpp's, at L = 1 and M = R0.  Pure functions of 64-bit indices.  No HIP:
// compiles with plain g++ (tests/ddc_wide_ring_check.cpp checks it under the host sanitizers).
//
// Indices are ABSOLUTE: input sample n counts from index 0 of the sample clock, intermediate sample k = n / R0 likewise.  The stream
// begins at n_origin (a multiple of 1008 rate / 12000, so k_origin = n_origin / R0 lies on the tile grid of the stage behind) and the
// input is zero before it.  Intermediate sample k is sum_j h0[j] u[k R0 + j - C0], C0 = (N0 - 1) / 2, N0 odd: its last input is
// k R0 + C0.
#pragma once
#include <cstdint>

#include "ddc_pre_ring.hpp"

namespace ddcwide {

constexpr int64_t RATE_MIN = 240000, RATE_MAX = 129600000;
constexpr int64_t MAX_R0 = 1350;            // largest first-stage decimation
constexpr int64_t MAX_TAPS = 8448;          // bound of len(h0) over every accepted rate (the longest: 48 kHz x 1349, about 8360 taps)
constexpr int64_t N_MAX = (int64_t)1 << 62; // bound of an origin

// the intermediate rate: the largest of 192000, 96000, 48000 that divides rate with R0 = rate / rate_mid >= 2; rate_mid = 0: refused
struct Plan { int64_t rate_mid, R0; };
constexpr Plan plan(int64_t rate) {
    if (rate < RATE_MIN || rate > RATE_MAX || rate % 48000 != 0) return Plan{0, 0};
    for (int64_t mid = 192000; mid >= 48000; mid /= 2)
        if (rate % mid == 0 && rate / mid >= 2) return rate / mid <= MAX_R0 ? Plan{mid, rate / mid} : Plan{0, 0};
    return Plan{0, 0};
}

// the kernel's tile (kernels/ddc_wide.hpp): the taps go through LDS in pieces of PIECE, the LDS image holds LDS_SAMPLES input samples,
// and a tile holds as many outputs (at most TILE_MAX) as fit next to one piece: (outputs - 1) R0 + PIECE <= LDS_SAMPLES
constexpr int64_t PIECE = 1024, LDS_SAMPLES = 6144, TILE_MAX = 16;
constexpr int64_t tile_outputs(int64_t R0) {
    const int64_t t = (LDS_SAMPLES - PIECE) / R0 + 1;
    return t < TILE_MAX ? t : TILE_MAX;
}

// samples of history the stream keeps: the next intermediate sample not yet made starts less than N0 - 1 + R0 before the newest input
constexpr int64_t history(int64_t N0, int64_t R0) { return N0 - 1 + R0; }

// the shared arithmetic under this stage's names and arguments: L = 1, M = R0
inline int64_t mid_done(int64_t n_origin, int64_t n_end, int64_t N0, int64_t R0) { return ddcpre::mid_done(n_origin, n_end, N0, 1, R0); }
inline int64_t mid_count(int64_t n_samples, int64_t N0, int64_t R0, int64_t cap) { return ddcpre::mid_count(n_samples, N0, 1, R0, cap); }
using ddcpre::hist_pos;
using ddcpre::Keep;
using ddcpre::keep;

}  // namespace ddcwide
