// ddc_ring.hpp -- the index arithmetic of the streaming down-converter (ft8rx_ddc_stream_*): which output
// tiles a push completes, where a chunk lands in the input ring, which outputs the output ring still holds.  Pure functions of
// 64-bit indices.  No HIP: compiles with plain g++ (tests/ddc_ring_check.cpp checks it under the host sanitizers).
//
// Indices are ABSOLUTE: input sample n and output sample m = n / D count from index 0 of the sample clock, the stream begins at
// n_origin (a multiple of TILE D, so m_origin = n_origin / D is a multiple of TILE) and the input is zero before it.  Output tile T
// holds m in [TILE T, TILE (T + 1)).
#pragma once
#include <cstdint>

namespace ddcring {

constexpr int64_t TILE = 1008;              // outputs per tile (kernels/ddc.hpp: DDC_TO)
constexpr int64_t OUT_RING = 360000;        // outputs the output ring holds per channel: two cycles

// the filter geometry at decimation D (kernels/ddc.hpp: DdcGeom; ft8rx.hip holds the two to each other by static_assert)
struct Geom { int64_t R1, C1, R2, C2; };
constexpr Geom geom(int D) {
    return Geom{D >= 4 ? D / 2 : 1, D == 4 ? 8 : D == 8 ? 15 : D == 16 ? 30 : 0, D == 1 ? 1 : 2, D == 1 ? 71 : 141};
}
// input samples a tile reaches BEFORE the first input of its first output (n = TILE D T): first input = TILE D T - back(D)
constexpr int64_t back(int D) { return geom(D).C2 * geom(D).R1 + geom(D).C1; }
// ... and the offset of the LAST input it needs from that same sample: last input = TILE D T + last(D)
constexpr int64_t last(int D) { return ((TILE - 1) * geom(D).R2 + geom(D).C2) * geom(D).R1 + geom(D).C1; }
// input samples under one tile
constexpr int64_t span(int D) { return back(D) + last(D) + 1; }

// capacity of the input ring per stream: the power of two that holds one second of input and one tile's span.  After a push every
// complete tile has been produced, so the oldest sample a later tile needs is less than span(D) behind the newest, and a push adds
// at most one second.
constexpr int64_t in_capacity(int D) {
    int64_t c = 1;
    while (c < 12000 * (int64_t)D + span(D)) c <<= 1;
    return c;
}

// absolute index of the first tile that is NOT complete when the inputs [.., n_end) exist: tile T is complete iff its last input,
// TILE D T + last(D), is below n_end.  Never below the origin's tile.
inline int64_t tiles_done(int64_t n_origin, int64_t n_end, int D) {
    const int64_t t0 = n_origin / (TILE * D), have = n_end - 1 - last(D);
    if (have < 0) return t0;
    const int64_t t = have / (TILE * D) + 1;
    return t > t0 ? t : t0;
}

// a chunk of n samples written at ring position pos (capacity cap, a power of two; n <= cap): the part up to the ring's end, the part
// that wraps to its start
struct Split { int64_t pos, first, second; };
inline Split split(int64_t written, int64_t n, int64_t cap) {
    const int64_t pos = written & (cap - 1), room = cap - pos;
    return Split{pos, n < room ? n : room, n < room ? 0 : n - room};
}

// position of absolute output m in the output ring (m may be negative only where the caller never stores)
inline int64_t out_pos(int64_t m) { const int64_t r = m % OUT_RING; return r < 0 ? r + OUT_RING : r; }

// the outputs [m_lo, m_hi) a gather or a read-back may still take from the ring: those of [m_first, m_first + n) that exist
// (m_origin <= m < m_done).  ok = false: part of them has been overwritten already (older than m_done - OUT_RING).
struct Range { int64_t lo, hi; bool ok; };
inline Range held(int64_t m_first, int64_t n, int64_t m_origin, int64_t m_done) {
    int64_t lo = m_first > m_origin ? m_first : m_origin, hi = m_first + n < m_done ? m_first + n : m_done;
    if (hi <= lo) return Range{lo, lo, true};
    return Range{lo, hi, lo >= m_done - OUT_RING};
}

}  // namespace ddcring
