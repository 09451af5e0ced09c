// ddc_wide_ring.hpp -- the index arithmetic of the wide pre-decimator (ft8rx_ddc_wide*): the plan of a rate,
// which intermediate samples a push completes, where a chunk lands in the history ring, how many outputs a tile of the kernel holds.
// Pure functions of 64-bit indices.  No HIP: compiles with plain g++ (tests/ddc_wide_ring_check.cpp checks it under the host
// sanitizers).
//
// Indices are ABSOLUTE: input sample n counts from index 0 of the sample clock, intermediate sample k = n / R0 likewise.  The stream
// begins at n_origin (a multiple of 1008 rate / 12000, so k_origin = n_origin / R0 lies on the tile grid of the stage behind) and the
// input is zero before it.  Intermediate sample k is sum_j h0[j] u[k R0 + j - C0], C0 = (N0 - 1) / 2, N0 odd: its last input is
// k R0 + C0.
#pragma once
#include <cstdint>

namespace ddcwide {

constexpr int64_t RATE_MIN = 240000, RATE_MAX = 129600000;
constexpr int64_t MAX_R0 = 1350;            // largest first-stage decimation
constexpr int64_t MAX_TAPS = 8448;          // bound of len(h0) over every accepted rate (the longest: 48 kHz x 1349, about 8360 taps)

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

// absolute index of the first intermediate sample that is NOT complete when the inputs [.., n_end) exist: k is complete iff its last
// input, k R0 + C0, is below n_end.  Never below the origin's sample.
inline int64_t mid_done(int64_t n_origin, int64_t n_end, int64_t N0, int64_t R0) {
    const int64_t k0 = n_origin / R0, have = n_end - 1 - (N0 - 1) / 2;
    if (have < 0) return k0;
    const int64_t k = have / R0 + 1;
    return k > k0 ? k : k0;
}

// intermediate samples of a one-shot call on n_samples inputs (zero outside): those a non-zero input can reach, at most `cap`
// (15 s at the intermediate rate), at least one
inline int64_t mid_count(int64_t n_samples, int64_t N0, int64_t R0, int64_t cap) {
    if (n_samples < 1) return 1;
    const int64_t k = (n_samples - 1 + (N0 - 1) / 2) / R0 + 1;
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

}  // namespace ddcwide
