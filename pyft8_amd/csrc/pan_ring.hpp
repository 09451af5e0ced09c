// pan_ring.hpp -- the index arithmetic of the panorama (ft8rx_pan*, kernels/pan.hpp): which windows and rows a
// push completes, where the leftover and the chunk sit in the work buffer, which rows the ring holds.  Pure functions of 64-bit
// indices.  No HIP: compiles with plain g++ (tests/pan_ring_check.cpp checks it under the host sanitizers).
//
// Indices are ABSOLUTE: sample n counts from index 0 of the sample clock, window w is the samples [w N, (w + 1) N), row r is the windows
// [r A, (r + 1) A).  The stream starts at n_origin; after a push its samples [n_origin, n_end) exist.  Only complete windows count and
// only complete rows exist: the first row is r_first, the first whose samples all lie in the stream, and the windows in front of it
// belong to no row and are never transformed.  A plan is a pure function of (n_origin, n_start, n_new, N, A): a stream keeps no other
// state than how many samples it has taken.
#pragma once
#include <cstdint>

namespace panring {

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// the first row that lies in the stream, and its first window
inline int64_t r_first(int64_t n_origin, int64_t N, int64_t A) { return ceil_div(ceil_div(n_origin, N), A); }
inline int64_t w_first(int64_t n_origin, int64_t N, int64_t A) { return r_first(n_origin, N, A) * A; }
// the first window that is NOT complete (or not wanted) when the samples [n_origin, n_end) exist, and the first such row
inline int64_t windows_done(int64_t n_origin, int64_t n_end, int64_t N, int64_t A) {
    const int64_t w = n_end / N, f = w_first(n_origin, N, A);
    return w > f ? w : f;
}
inline int64_t rows_done(int64_t n_origin, int64_t n_end, int64_t N, int64_t A) { return windows_done(n_origin, n_end, N, A) / A; }

// The ring: n_rows + 1 slots, row r at r mod (n_rows + 1) -- the newest n_rows finished rows and the one in progress, which
// accumulates in its own slot.
inline int64_t slots(int64_t n_rows) { return n_rows + 1; }
struct Held { int64_t r_lo, r_hi; };       // the finished rows [r_lo, r_hi) can be read
inline Held held(int64_t n_origin, int64_t n_end, int64_t N, int64_t A, int64_t n_rows) {
    Held h;
    h.r_hi = rows_done(n_origin, n_end, N, A);
    const int64_t f = r_first(n_origin, N, A);
    h.r_lo = h.r_hi - n_rows > f ? h.r_hi - n_rows : f;
    return h;
}

// samples of the work buffer of a stream whose pushes carry at most max_push samples: the leftover (< N) and the chunk
inline int64_t capacity(int64_t N, int64_t max_push) { return N - 1 + max_push; }
// windows of one launch pair (power, rows): at most tile_cap, and so few that they touch at most n_rows + 1 rows = distinct slots
inline int64_t tile_windows(int64_t tile_cap, int64_t n_rows, int64_t A) { return tile_cap < n_rows * A ? tile_cap : n_rows * A; }

// One push of n_new samples behind [n_origin, n_start).
//   base       absolute index of the work buffer's first sample
//   left_n     leftover samples [base, n_start) kept from the pushes before, at position 0; the chunk follows at chunk_at = n_start - base
//   w0, w1     the windows this push transforms; window w0 starts at position first_at = w0 N - base (meaningless when w1 == w0)
//   r0, r1     the rows it finishes
//   keep_n     samples [n_end - keep_n, n_end) the next push needs: its leftover, at position keep_at
struct Plan { int64_t base, left_n, chunk_at, w0, w1, first_at, r0, r1, keep_n, keep_at, n_end; };
inline Plan plan(int64_t n_origin, int64_t n_start, int64_t n_new, int64_t N, int64_t A) {
    Plan p;
    p.n_end = n_start + n_new;
    p.w0 = windows_done(n_origin, n_start, N, A);
    p.w1 = windows_done(n_origin, p.n_end, N, A);
    p.r0 = p.w0 / A;
    p.r1 = p.w1 / A;
    const int64_t keep = p.w0 * N;                       // the first sample a window still needs
    p.left_n = keep < n_start ? n_start - keep : 0;
    p.base = n_start - p.left_n;
    p.chunk_at = p.left_n;
    p.first_at = keep - p.base;
    const int64_t keep_next = p.w1 * N;
    p.keep_n = keep_next < p.n_end ? p.n_end - keep_next : 0;
    p.keep_at = p.n_end - p.keep_n - p.base;
    return p;
}

}  // namespace panring
