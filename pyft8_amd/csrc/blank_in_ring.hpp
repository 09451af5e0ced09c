// blank_in_ring.hpp -- the index arithmetic of the input-rate noise blanker (ft8rx_blank_in*,
// kernels/blank_in.hpp): which samples are final after a push, which blocks a push completes, where the leftover and the new samples
// sit in the work buffer.  Pure functions of 64-bit indices.  No HIP: compiles with plain g++ (tests/blank_in_ring_check.cpp checks it
// under the host sanitizers).
//
// Indices are ABSOLUTE: sample n counts from index 0 of the sample clock, block b is [b B, (b + 1) B), B a power of two.  The stream
// starts at n_origin; after a push its samples [n_origin, n_end) exist.  A plan is a pure function of (n_origin, n_start, n_new,
// finish): a stream keeps no other state than how many samples it has taken.
#pragma once
#include <cstdint>

namespace blankin {

// Sample n is final once every block up to (n + G + R) / B + 2 is complete, i.e. n < (n_end / B - 2) B - (G + R): the first sample
// that is NOT final when the inputs [.., n_end) exist, never below the origin.
inline int64_t released(int64_t n_origin, int64_t n_end, int64_t B, int64_t G, int64_t R) {
    const int64_t r = (n_end / B - 2) * B - (G + R);
    return r > n_origin ? r : n_origin;
}

// samples of the work buffer (either of the two) of a stream whose pushes carry at most max_push samples: the slack below a block
// start (< B), the leftover (< 3 B + G + R) and the chunk
inline int64_t capacity(int64_t B, int64_t G, int64_t R, int64_t max_push) { return 4 * B + G + R + max_push; }

// One push of n_new samples behind [n_origin, n_start); finish: everything beyond n_start + n_new is outside the stream.
//   base       absolute index of the work buffer's first sample: the block start at or below the first sample it keeps
//   left_n     leftover samples [g0, n_start), at position g0 - base; the chunk follows them at n_start - base
//   lv0, lv1   blocks whose level m_b this push makes (finish: the partial tail block too)
//   hb0, hb1   blocks whose hits it derives: m of b + 2 exists (finish: blocks beyond the stream have m = 0)
//   g0, g1     samples it gates and releases
//   b_first    the block of the origin; b_have: blocks [b_first, b_have) have a level after this push
//   m_hi       the hit mask is known on [b_first B, m_hi) after this push (zero outside the stream)
struct Plan { int64_t base, left_n, lv0, lv1, hb0, hb1, g0, g1, b_first, b_have, m_hi, n_end; };
inline Plan plan(int64_t n_origin, int64_t n_start, int64_t n_new, bool finish, int64_t B, int64_t G, int64_t R) {
    Plan p;
    p.n_end = n_start + n_new;
    p.b_first = n_origin / B;
    const int64_t c0 = n_start / B, c1 = p.n_end / B, tail = finish ? (p.n_end + B - 1) / B : c1;
    p.g0 = released(n_origin, n_start, B, G, R);
    p.g1 = finish ? p.n_end : released(n_origin, p.n_end, B, G, R);
    p.base = p.g0 / B * B;
    p.left_n = n_start - p.g0;
    p.lv0 = c0 > p.b_first ? c0 : p.b_first;
    p.lv1 = tail;
    p.hb0 = c0 - 2 > p.b_first ? c0 - 2 : p.b_first;
    p.hb1 = finish ? tail : (c1 - 2 > p.hb0 ? c1 - 2 : p.hb0);
    p.b_have = tail;
    p.m_hi = p.hb1 * B;
    return p;
}

}  // namespace blankin
