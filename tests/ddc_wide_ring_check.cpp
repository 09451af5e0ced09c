// ddc_wide_ring_check.cpp -- stand-alone check of the wide pre-decimator's index arithmetic (pyft8_amd/csrc/ddc_wide_ring.hpp), built
// with g++ -fsanitize=address,undefined and run on the CPU by tests/test_ddc_wide.py.  It replays pushes of 1, R0 - 1, R0, a prime and
// one second of samples against a model of the history ring and checks, for six rates: the count of complete intermediate samples
// against its definition, that every input a new intermediate sample reads lies before the origin, in the chunk or still in the ring
// at the position the kernel computes (kernels/ddc_wide.hpp: k_ddc_pre_stream), and the split of the history update -- at the origin,
// across n = 2^32 and at 2^50.  Then the plans, the tile sizes and the one-shot count, and the shared forms of ddc_pre_ring.hpp at
// L = 1, M = R0 against the wide stage's own closed forms and its modulus rule for an origin.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pyft8_amd/csrc/ddc_wide_ring.hpp"

using namespace ddcwide;

static long checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { fprintf(stderr, "ddc_wide_ring_check: %s failed (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static void check_stream(int64_t rate, int64_t N0, int64_t n_origin, uint32_t seed) {
    const Plan p = plan(rate);
    CHECK(p.rate_mid > 0 && p.R0 * p.rate_mid == rate);
    const int64_t R0 = p.R0, C0 = (N0 - 1) / 2, H = history(N0, R0), grid = 1008 * (rate / 12000);
    CHECK(n_origin % grid == 0 && n_origin % R0 == 0 && (n_origin / R0) % (1008 * (p.rate_mid / 12000)) == 0);
    std::vector<int64_t> ring((size_t)H, -1);            // the absolute index each cell of the history holds
    int64_t pushed = 0, k_done = n_origin / R0;
    CHECK(mid_done(n_origin, n_origin, N0, R0) == k_done);
    const int64_t lens[6] = {1, R0 - 1, R0, 7919, rate, 2 * R0 + 1};
    for (int step = 0; step < 300; step++) {
        seed = seed * 1664525u + 1013904223u;
        const int64_t n_new = lens[(seed >> 24) % 6];
        const int64_t n_start = n_origin + pushed, n_end = n_start + n_new;
        const int64_t k_new = mid_done(n_origin, n_end, N0, R0);
        CHECK(k_new >= k_done && k_new - k_done <= p.rate_mid);              // a push makes at most a second of intermediate samples
        CHECK(k_new == n_origin / R0 || (k_new - 1) * R0 + C0 < n_end);      // the definition: k is complete iff its last input exists
        CHECK(k_new * R0 + C0 >= n_end);
        if (n_new < R0 && step > 0) CHECK(k_new - k_done <= 1);
        // what the kernel reads for the new samples, before the history is updated
        const int64_t p_last = pushed ? hist_pos(n_start - 1, n_origin, H) : 0;
        for (int64_t k = k_done; k < k_new; k += (k < k_done + 2 || k >= k_new - 3) ? 1 : (k_new - k_done) / 5 + 1) {
            const int64_t n0 = k * R0 - C0, n1 = k * R0 + C0;
            CHECK(n1 < n_end && n1 - n0 + 1 == N0);
            for (int64_t n = n0; n <= n1; n += (n < n0 + 3 || n > n1 - 4) ? 1 : 97) {
                if (n < n_origin || n >= n_start) continue;                  // zero, or in the chunk
                const int64_t d = n_start - 1 - n;
                CHECK(d >= 0 && d < H);
                const int64_t q = p_last - d < 0 ? p_last - d + H : p_last - d;
                CHECK(q >= 0 && q < H && ring[(size_t)q] == n && q == hist_pos(n, n_origin, H));
            }
        }
        // the history update: the chunk's last min(n_new, H) samples, in at most two pieces
        const Keep kp = keep(pushed, n_new, H);
        CHECK(kp.skip >= 0 && kp.first >= 1 && kp.second >= 0 && kp.skip + kp.first + kp.second == n_new && kp.first + kp.second <= H);
        CHECK(kp.pos >= 0 && kp.pos + kp.first <= H && kp.second <= kp.pos && (kp.skip == 0 || kp.first + kp.second == H));
        for (int64_t i = 0; i < kp.first; i++) ring[(size_t)(kp.pos + i)] = n_start + kp.skip + i;
        for (int64_t i = 0; i < kp.second; i++) ring[(size_t)i] = n_start + kp.skip + kp.first + i;
        pushed += n_new;
        k_done = k_new;
        // the newest min(pushed, H) samples are all there, each at its position
        for (int64_t n = n_end - 1; n >= n_origin && n > n_end - 1 - H; n -= (n > n_end - 4 || n < n_end - H + 3) ? 1 : 89)
            CHECK(ring[(size_t)hist_pos(n, n_origin, H)] == n);
        // ... and the next sample not yet made needs nothing older
        CHECK(k_done * R0 - C0 > n_end - 1 - H || k_done * R0 - C0 < n_origin);
    }
}

// The closed forms the wide header had before the shared arithmetic of ddc_pre_ring.hpp took their place, written out here so that the
// expected values do not come from the code under test
static int64_t wide_mid_done(int64_t n_origin, int64_t n_end, int64_t N0, int64_t R0) {
    const int64_t k0 = n_origin / R0, have = n_end - 1 - (N0 - 1) / 2;
    if (have < 0) return k0;
    const int64_t k = have / R0 + 1;
    return k > k0 ? k : k0;
}
static int64_t wide_mid_count(int64_t n_samples, int64_t N0, int64_t R0, int64_t cap) {
    if (n_samples < 1) return 1;
    const int64_t k = (n_samples - 1 + (N0 - 1) / 2) / R0 + 1;
    return k < cap ? k : cap;
}
static bool wide_origin_ok(uint64_t n_origin, int64_t rate) {
    return n_origin % (uint64_t)(1008 * (rate / 12000)) == 0 && n_origin <= ((uint64_t)1 << 62);
}

// the shared forms at L = 1, M = R0 against those, around tile and tap boundaries
static void check_shared_forms(int64_t rate, int64_t N0) {
    const Plan p = plan(rate);
    const int64_t R0 = p.R0, C0 = (N0 - 1) / 2, tk = tile_outputs(R0), grid = 1008 * (rate / 12000), cap = 180000 * (p.rate_mid / 12000);
    const int64_t origins[4] = {0, grid, 5 * grid, ((int64_t)1 << 40) / grid * grid};
    const int64_t around[8] = {0, C0, N0, R0, tk * R0, tk * R0 + C0, 3 * tk * R0 - C0 + N0, grid};
    for (int64_t o : origins) {
        CHECK(ddcpre::k_origin(o, 1, R0) == o / R0 && ddcpre::k_origin(o, 1, R0) * R0 == o);
        for (int64_t a : around)
            for (int64_t d = -2; d <= 2; d++) {
                const int64_t n_end = o + a + d;
                if (n_end >= 0) CHECK(ddcpre::mid_done(o, n_end, N0, 1, R0) == wide_mid_done(o, n_end, N0, R0));
                const int64_t n = a + d;
                CHECK(ddcpre::mid_count(n, N0, 1, R0, cap) == wide_mid_count(n, N0, R0, cap));
                CHECK(ddcpre::mid_count(n, N0, 1, R0, 7) == wide_mid_count(n, N0, R0, 7));
                // the origin rule: n_origin L / M an integer on the tile grid of the stage behind == a multiple of 1008 rate / 12000
                const int64_t cand = o + (a % 3 == 0 ? a : R0 * a) + d;
                if (cand >= 0) CHECK(ddcpre::origin_ok(cand, N_MAX, p.rate_mid, 1, R0) == wide_origin_ok((uint64_t)cand, rate));
            }
        CHECK(ddcpre::origin_ok(o, N_MAX, p.rate_mid, 1, R0) && !ddcpre::origin_ok(o + R0, N_MAX, p.rate_mid, 1, R0) && !ddcpre::origin_ok(o + grid / 2, N_MAX, p.rate_mid, 1, R0));
    }
    CHECK(!ddcpre::origin_ok(-grid, N_MAX, p.rate_mid, 1, R0) && !ddcpre::origin_ok(N_MAX / grid * grid + grid, N_MAX, p.rate_mid, 1, R0));
    CHECK(ddcpre::origin_ok(N_MAX / grid * grid, N_MAX, p.rate_mid, 1, R0) == wide_origin_ok((uint64_t)(N_MAX / grid * grid), rate));
}

int main() {
    const int64_t rates[6] = {240000, 384000, 768000, 2400000, 64800000, 129600000};
    const int64_t mids[6] = {48000, 192000, 192000, 96000, 96000, 192000}, r0s[6] = {5, 2, 4, 25, 675, 675};
    const int64_t taps[6] = {33, 13, 25, 145, 3883, 3749};
    const int64_t two32 = (int64_t)1 << 32;
    for (int i = 0; i < 6; i++) {
        const Plan p = plan(rates[i]);
        CHECK(p.rate_mid == mids[i] && p.R0 == r0s[i]);
        const int64_t grid = 1008 * (rates[i] / 12000);
        check_stream(rates[i], taps[i], 0, 1u + i);
        check_stream(rates[i], taps[i], grid * 3, 2u + i);
        check_stream(rates[i], taps[i], (two32 - 2 * grid - 1) / grid * grid, 3u + i);          // the pushes cross n = 2^32
        check_stream(rates[i], taps[i], ((int64_t)1 << 50) / grid * grid, 4u + i);
    }
    check_stream(48000 * 1349, MAX_TAPS - 1, 0, 99u);                                           // the longest filter, the largest R0
    const int64_t refused[9] = {250000, 2048000, 192000, 144000, 129648000, 0, -240000, 239999, 48000 * 1351 * 2 + 48000};
    for (int64_t r : refused) CHECK(plan(r).rate_mid == 0 && plan(r).R0 == 0);
    CHECK(plan(48000 * 1349).rate_mid == 48000 && plan(48000 * 1351).rate_mid == 0 && plan(96000 * 1351).rate_mid == 0);
    // every accepted rate: R0 >= 2 within the limit, the largest intermediate rate that divides
    for (int64_t r = RATE_MIN; r <= RATE_MAX; r += 48000) {
        const Plan p = plan(r);
        if (!p.rate_mid) { CHECK(r / 48000 > MAX_R0 && (r % 96000 != 0 || r / 96000 > MAX_R0) && (r % 192000 != 0 || r / 192000 > MAX_R0)); continue; }
        CHECK(p.R0 >= 2 && p.R0 <= MAX_R0 && p.R0 * p.rate_mid == r);
        CHECK(p.rate_mid == 192000 || r % (2 * p.rate_mid) != 0 || r / (2 * p.rate_mid) < 2);
    }
    // the kernel's tile: at least one output, and the inputs under one piece of taps fit the LDS image
    for (int64_t r = 2; r <= MAX_R0; r++) {
        const int64_t t = tile_outputs(r);
        CHECK(t >= 1 && t <= TILE_MAX && (t - 1) * r + PIECE <= LDS_SAMPLES && (t == TILE_MAX || t * r + PIECE > LDS_SAMPLES));
    }
    // the one-shot count: the samples a non-zero input can reach, capped, at least one
    CHECK(mid_count(0, 33, 5, 720000) == 1 && mid_count(1, 33, 5, 720000) == 4 && mid_count(5, 33, 5, 720000) == 5);
    CHECK(mid_count(3600000, 33, 5, 720000) == 720000 && mid_count(3600000 - 1237, 33, 5, 720000) == 719756);
    for (int64_t n = 1; n < 400; n++) {
        const int64_t k = mid_count(n, 33, 5, 1 << 30);
        CHECK((k - 1) * 5 - 16 <= n - 1 && k * 5 - 16 > n - 1);                                // k - 1 still reaches the last input, k does not
    }
    // the shared arithmetic at L = 1, M = R0 is the wide stage's own: a small sweep of accepted R0 (N0 = 6 R0 + 1 or + 3, odd, like the designs)
    for (int i = 0; i < 6; i++) check_shared_forms(rates[i], taps[i]);
    for (int64_t r = RATE_MIN; r <= RATE_MAX; r += 48000 * 37) {
        const Plan p = plan(r);
        if (p.rate_mid) check_shared_forms(r, (6 * p.R0 + 1) | 1);
    }
    printf("ddc wide ring arithmetic: %ld checked\n", checks);
    return 0;
}
