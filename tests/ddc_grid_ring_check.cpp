// ddc_grid_ring_check.cpp -- stand-alone check of the index arithmetic of the spectrogram stage behind the streaming down-converter
// (pyft8_amd/csrc/ddc_grid_ring.hpp), built with g++ -fsanitize=address,undefined and run on the CPU by tests/test_ddc_grid.py.  It
// replays pushes (m_produced advancing in whole tiles of 1008, 0 .. 12 of them at a time) against a plain model -- the output ring as
// an array of the absolute index each cell holds, the grid ring as an array of the row each slot holds -- and walks every window as
// k_grid_stream does (first slot of the first hop, 480 more per hop, one compare and subtract per wrap): at the origin, with p0 in
// {0, 1, 137, 479}, across the output ring's wrap, across the grid ring's wrap, and at m near 2^50.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pyft8_amd/csrc/ddc_grid_ring.hpp"

using namespace ddcgrid;

static long checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { fprintf(stderr, "ddc_grid_ring_check: %s failed (line %d)\n", #c, __LINE__); exit(1); } } while (0)

constexpr int64_t TILE = 1008;

static void check_stream(int64_t m_origin, int64_t p0, int64_t n_rows, int steps, uint32_t seed) {
    CHECK(m_origin % TILE == 0 && p0 >= 0 && p0 < HOP && n_rows >= MIN_ROWS && n_rows <= MAX_ROWS);
    std::vector<int64_t> ring((size_t)OUT_RING, -1);          // the absolute output index each cell of the output ring holds
    std::vector<int64_t> grid((size_t)n_rows, -1);            // the row each slot of the grid ring holds
    int64_t m = m_origin;
    // the definition of a row, by brute force: the first q with p0 + HOP q > m_origin
    int64_t q0 = (m_origin - p0) / HOP - 2;
    if (q0 < 0) q0 = 0;
    while (p0 + HOP * q0 <= m_origin) q0++;
    CHECK(q0 == 0 || p0 + HOP * (q0 - 1) <= m_origin);
    CHECK(hops_done(m_origin, p0) == q0);
    int64_t next = q0;                                        // the model's next row
    for (int step = 0; step < steps; step++) {
        seed = seed * 1664525u + 1013904223u;
        const int64_t tiles = (seed >> 24) % 13, m_new = m + TILE * tiles;
        for (int64_t k = m; k < m_new; k++) ring[(size_t)(k % OUT_RING)] = k;
        const Hops hp = completed(m, m_new, p0, m_origin, n_rows);
        // the definition: hop q is complete iff p0 + HOP q <= m_produced
        int64_t end = next;
        while (p0 + HOP * end <= m_new) end++;
        CHECK(hp.end == end && hp.first <= hp.end && hp.end - hp.first <= n_rows);
        CHECK(hp.first == (end - next > n_rows ? end - n_rows : next));
        if (hp.end > hp.first) {                              // the launch: what the host hands over for the FIRST hop ...
            int64_t slot = window_slot(hp.first, p0), nz = zero_prefix(hp.first, p0, m_origin), row = row_slot(hp.first, n_rows);
            CHECK(slot >= 0 && slot < OUT_RING && nz >= 0 && nz < WIN && row >= 0 && row < n_rows);
            CHECK(HOP * (hp.end - hp.first) <= OUT_RING);
            for (int64_t q = hp.first; q < hp.end; q++) {     // ... and what block q - hp.first makes of it
                const int64_t b = q - hp.first;
                int64_t s = slot + HOP * b, r = row + b, z = nz - HOP * b;
                if (s >= OUT_RING) s -= OUT_RING;
                if (r >= n_rows) r -= n_rows;
                if (z < 0) z = 0;
                CHECK(s == window_slot(q, p0) && r == row_slot(q, n_rows) && z == zero_prefix(q, p0, m_origin));
                CHECK(window_wraps(q, p0) == (s + WIN > OUT_RING));
                const int64_t w0 = window_first(q, p0);
                CHECK(w0 + WIN == p0 + HOP * q && w0 + WIN <= m_new && w0 + WIN > m_origin);
                for (int64_t i = 0; i < WIN; i += (i < 3 || i > WIN - 4 || (i >= z - 2 && i <= z + 2) || (s + i >= OUT_RING - 2 && s + i <= OUT_RING + 2)) ? 1 : 53) {
                    int64_t at = s + i;
                    if (at >= OUT_RING) at -= OUT_RING;
                    CHECK(at >= 0 && at < OUT_RING);
                    if (i < z) CHECK(w0 + i < m_origin);                      // masked: before the origin
                    else CHECK(w0 + i >= m_origin && ring[(size_t)at] == w0 + i);      // in the ring, written, not yet overwritten
                }
                grid[(size_t)r] = q;
            }
        }
        next = end;
        m = m_new;
        const Held hd = held(m, p0, m_origin, n_rows);
        CHECK(hd.next == next && hd.first == (next - n_rows > q0 ? next - n_rows : q0) && hd.first <= hd.next);
        for (int64_t q = hd.first; q < hd.next; q++) CHECK(grid[(size_t)row_slot(q, n_rows)] == q);       // every held row is where it is read
    }
    CHECK(next > q0);
}

int main() {
    const int64_t p0s[4] = {0, 1, 137, 479};
    uint32_t seed = 1;
    for (int64_t p0 : p0s) {
        check_stream(0, p0, 750, 120, seed++);                                  // at the origin: windows that reach before it
        check_stream(0, p0, 16, 60, seed++);                                    // the grid ring wraps at once, and a push brings more rows than it holds
        check_stream(TILE * 357, p0, 16, 40, seed++);                           // m passes OUT_RING inside the first window
        check_stream(TILE * 350, p0, 750, 140, seed++);                         // both rings wrap
        check_stream(((int64_t)1 << 50) / TILE * TILE, p0, 750, 140, seed++);   // m near 2^50
        check_stream(((int64_t)1 << 50) / TILE * TILE + TILE * 5, p0, 17, 60, seed++);
    }
    // hop 0 is no row of a stream that begins at 0 with p0 = 0 (its window holds nothing of the stream); with p0 > 0 it is
    CHECK(hops_done(0, 0) == 1 && hops_done(0, 1) == 0 && hops_done(479, 479) == 1 && hops_done(478, 479) == 0 && hops_done(480, 0) == 2);
    CHECK(window_first(1, 0) == -3360 && window_slot(1, 0) == OUT_RING - 3360 && window_wraps(1, 0) && zero_prefix(1, 0, 0) == 3360);
    CHECK(window_first(8, 0) == 0 && window_slot(8, 0) == 0 && !window_wraps(8, 0) && zero_prefix(8, 0, 0) == 0);
    CHECK(zero_prefix(0, 137, 0) == 3703 && zero_prefix(100, 137, 0) == 0);
    CHECK(window_slot(750, 0) == OUT_RING - WIN && !window_wraps(750, 0) && window_wraps(751, 0));
    Hops h = completed(0, 0, 0, 0, 750);
    CHECK(h.first == h.end);                                                    // nothing produced: nothing launched
    h = completed(1008, 1008, 5, 0, 750);
    CHECK(h.first == h.end);
    h = completed(0, 12096, 0, 0, 16);
    CHECK(h.end == 26 && h.first == 10);                                        // 25 new rows, 16 kept
    Held d = held(0, 0, 0, 16);
    CHECK(d.first == d.next && d.next == 1);
    printf("ddc grid ring arithmetic: %ld checked\n", checks);
    return 0;
}
