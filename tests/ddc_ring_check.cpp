// ddc_ring_check.cpp -- stand-alone check of the streaming down-converter's index arithmetic (pyft8_amd/csrc/ddc_ring.hpp), built
// with g++ -fsanitize=address,undefined and run on the CPU by tests/test_ddc_stream.py.  It replays pushes of irregular lengths against
// a byte-level model of the input ring and checks, for every D: the tile count against its definition by brute force, that every
// sample a produced tile reads is still in the ring and was written by the split copies, the output ring positions, and the range
// rule of the gather -- around the origin, around n = 2^32 and at negative output indices.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pyft8_amd/csrc/ddc_ring.hpp"

using namespace ddcring;

static long checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { fprintf(stderr, "ddc_ring_check: %s failed (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static void check_stream(int D, int64_t n_origin, uint32_t seed) {
    const int64_t cap = in_capacity(D), rate = 12000 * (int64_t)D;
    CHECK((cap & (cap - 1)) == 0 && cap >= rate + span(D) && cap / 2 < rate + span(D));
    CHECK(n_origin % (TILE * D) == 0);
    std::vector<int64_t> ring((size_t)cap, -1);          // the absolute index each ring cell holds
    int64_t pushed = 0, tiles = n_origin / (TILE * D);
    CHECK(tiles_done(n_origin, n_origin, D) == tiles);
    const int64_t lens[6] = {1, 479, 480 * D, 7 * D + 3, rate, rate - 1};
    for (int step = 0; step < 400; step++) {
        seed = seed * 1664525u + 1013904223u;
        const int64_t n = lens[(seed >> 24) % 6];
        const Split s = split(pushed, n, cap);
        CHECK(s.first >= 1 && s.second >= 0 && s.first + s.second == n && s.pos >= 0 && s.pos + s.first <= cap && s.second <= s.pos);
        for (int64_t i = 0; i < s.first; i++) ring[(size_t)(s.pos + i)] = n_origin + pushed + i;
        for (int64_t i = 0; i < s.second; i++) ring[(size_t)i] = n_origin + pushed + s.first + i;
        pushed += n;
        const int64_t n_end = n_origin + pushed, done = tiles_done(n_origin, n_end, D);
        CHECK(done >= tiles && done - tiles <= 12000 / TILE + 2);
        // the definition: tile T is complete iff its last input exists
        CHECK(done == n_origin / (TILE * D) || TILE * D * (done - 1) + last(D) < n_end);
        CHECK(TILE * D * done + last(D) >= n_end);
        for (int64_t T = tiles; T < done; T++) {         // every input of a new tile: before the origin (zero) or still in the ring
            const int64_t n0 = TILE * D * T - back(D), n1 = TILE * D * T + last(D);
            CHECK(n1 - n0 + 1 == span(D) && n1 < n_end);
            for (int64_t k = n0; k <= n1; k += (k < n0 + 3 || k > n1 - 3) ? 1 : 97)
                CHECK(k < n_origin || ring[(size_t)((k - n_origin) & (cap - 1))] == k);
        }
        tiles = done;
    }
}

int main() {
    const int Ds[5] = {1, 2, 4, 8, 16};
    for (int D : Ds) {
        const Geom g = geom(D);
        CHECK(g.R1 * g.R2 == D && back(D) == g.C2 * g.R1 + g.C1);
        check_stream(D, 0, 1u + D);
        check_stream(D, TILE * D * 7, 2u + D);
        // the largest multiple of 1008 D below 2^32 - 2 x 1008 D: the pushes cross n = 2^32
        const int64_t two32 = (int64_t)1 << 32;
        check_stream(D, (two32 - 2 * TILE * D - 1) / (TILE * D) * (TILE * D), 3u + D);
        check_stream(D, ((int64_t)1 << 50) / (TILE * D) * (TILE * D), 4u + D);
    }
    // output ring positions
    CHECK(out_pos(0) == 0 && out_pos(OUT_RING) == 0 && out_pos(OUT_RING + 5) == 5 && out_pos(-1) == OUT_RING - 1 && out_pos(-OUT_RING) == 0);
    CHECK(out_pos(((int64_t)1 << 40) + 3) == (((int64_t)1 << 40) + 3) % OUT_RING);
    // the gather's range rule: (m_first, n, m_origin, m_done)
    Range r = held(-6000, 180000, 0, 1008 * 200);
    CHECK(r.ok && r.lo == 0 && r.hi == 174000);                                      // a zero head before the origin
    r = held(1, 180000, 0, 1008 * 100);
    CHECK(r.ok && r.lo == 1 && r.hi == 100800);                                      // odd start, zero tail beyond the outputs produced
    r = held(300001, 180000, 0, 1008 * 400);
    CHECK(r.ok && r.lo == 300001 && r.hi == 403200);                                 // wraps the ring: still held
    r = held(1008 * 400 - 360000, 10, 0, 1008 * 400);
    CHECK(r.ok);                                                                     // the oldest output held
    r = held(1008 * 400 - 360000 - 1, 10, 0, 1008 * 400);
    CHECK(!r.ok);                                                                    // one older: it has left the ring
    r = held(0, 180000, 0, 1008 * 600);
    CHECK(!r.ok);
    r = held(-200000, 180000, 0, 1008 * 600);
    CHECK(r.ok && r.lo == r.hi);                                                     // wholly before the origin: all zero, nothing read
    r = held(1008 * 700, 500, 0, 1008 * 600);
    CHECK(r.ok && r.lo == r.hi);                                                     // wholly beyond the outputs produced
    r = held(5, 0, 0, 1008 * 600);
    CHECK(r.ok && r.lo == r.hi);
    printf("ddc ring arithmetic: %ld checked\n", checks);
    return 0;
}
