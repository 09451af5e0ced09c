// ddc_grid_ring.hpp -- the index arithmetic of the spectrogram stage behind the streaming down-converter (DESIGN.md section 16.5;
// ft8rx_ddc_stream_grid_*): which hops a push completes, where a hop's window lies in the output ring, how much of it lies before the
// stream's origin, which rows the grid ring still holds.  Pure functions of 64-bit indices.  No HIP: compiles with plain g++
// (tests/ddc_grid_ring_check.cpp checks it under the host sanitizers).
//
// Indices are ABSOLUTE, as in ddc_ring.hpp: output m counts from index 0 of the 12 kHz sample clock, the stream's first output is
// m_origin and the outputs before it are zeros.  With the grid open at hop phase p0 (0 <= p0 < HOP), hop q ends at e(q) = p0 + HOP q:
// its window is the outputs [e(q) - WIN, e(q)).  Hop q is a ROW iff e(q) > m_origin (its window holds at least one output of the
// stream), and it is complete once e(q) <= m_produced.
#pragma once
#include <cstdint>

namespace ddcgrid {

constexpr int64_t HOP = 480;                // outputs per hop (kernels/spectrogram.hpp)
constexpr int64_t WIN = 3840;               // outputs per window
constexpr int64_t OUT_RING = 360000;        // outputs the down-converter's output ring holds per channel (ddc_ring.hpp)
constexpr int64_t MIN_ROWS = 16, MAX_ROWS = 750;      // rows the grid ring may hold per channel (750: two cycles)

// the first hop that does NOT end inside [.., m): the number of q >= 0 with p0 + HOP q <= m.  m >= 0.
inline int64_t hops_done(int64_t m, int64_t p0) { return m < p0 ? 0 : (m - p0) / HOP + 1; }

// the hops [first, end) a push completes that moved m_produced from m_before to m_after: never a hop that is no row (before the
// origin), and of more than n_rows new hops only the newest n_rows (the others would be overwritten in the grid ring at once)
struct Hops { int64_t first, end; };
inline Hops completed(int64_t m_before, int64_t m_after, int64_t p0, int64_t m_origin, int64_t n_rows) {
    const int64_t q0 = hops_done(m_origin, p0), end = hops_done(m_after, p0);
    int64_t first = hops_done(m_before, p0);
    if (first < q0) first = q0;
    if (first < end - n_rows) first = end - n_rows;
    return Hops{first < end ? first : end, end};
}

// absolute index of the first output of hop q's window (negative for the first hops of a stream that begins at index 0)
inline int64_t window_first(int64_t q, int64_t p0) { return p0 + HOP * q - WIN; }
// ... its slot in the output ring, and whether the window runs past the ring's end (then it goes on at slot 0)
inline int64_t window_slot(int64_t q, int64_t p0) { const int64_t r = window_first(q, p0) % OUT_RING; return r < 0 ? r + OUT_RING : r; }
inline bool window_wraps(int64_t q, int64_t p0) { return window_slot(q, p0) + WIN > OUT_RING; }
// ... and how many of its first outputs lie before the origin (zeros): 0 .. WIN
inline int64_t zero_prefix(int64_t q, int64_t p0, int64_t m_origin) {
    const int64_t z = m_origin - window_first(q, p0);
    return z < 0 ? 0 : z > WIN ? WIN : z;
}

// the rows [first, next) the grid ring holds when the outputs [.., m_done) exist: the newest n_rows of the rows completed so far
struct Held { int64_t first, next; };
inline Held held(int64_t m_done, int64_t p0, int64_t m_origin, int64_t n_rows) {
    const int64_t q0 = hops_done(m_origin, p0), next = hops_done(m_done, p0);
    const int64_t first = next - n_rows > q0 ? next - n_rows : q0;
    return Held{first < next ? first : next, next};
}

// slot of row q in the grid ring (q >= 0)
inline int64_t row_slot(int64_t q, int64_t n_rows) { return q % n_rows; }

}  // namespace ddcgrid
