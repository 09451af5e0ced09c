// ddc_rat_ring_check.cpp -- stand-alone check of the rational resampler's index arithmetic (pyft8_amd/csrc/ddc_rat_ring.hpp), built with
// g++ -fsanitize=address,undefined and run on the CPU by tests/test_ddc_rat.py.  It replays pushes of 1, M - 1, M, a prime and one
// second of samples against a brute-force model (a counter that walks k up while its last input exists, and a model of the history
// ring) for the plans 160/147, 24/125, 3/32 and 3/625 -- at the origin, across n = 2^32 and at n of about 2^50 -- and checks that the
// set of complete intermediate samples never skips or repeats, that every input a new sample reads lies before the origin, in the
// chunk or still in the ring at the position the kernel computes (kernels/ddc_rat.hpp: k_ddc_rat_stream), and the split of the
// history update.  Then the plans, the origin rule, the tile sizes of both regimes and the one-shot count.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pyft8_amd/csrc/ddc_rat_ring.hpp"

using namespace ddcrat;

static long checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { fprintf(stderr, "ddc_rat_ring_check: %s failed (line %d)\n", #c, __LINE__); exit(1); } } while (0)

// the first valid origin at or above n: n_origin L / M on the grid of 1008 rate_mid / 12000
static int64_t origin_at(int64_t n, const Plan& p) {
    const int64_t gk = 1008 * (p.rate_mid / 12000);          // the grid in k; k M / L must be an integer as well
    int64_t step = gk;
    while ((step * p.M) % p.L) step += gk;                  // the smallest multiple of gk whose input time is an integer
    const int64_t gn = step * p.M / p.L;
    return (n + gn - 1) / gn * gn;
}

static void check_stream(int64_t rate, int64_t N, int64_t n_origin, uint32_t seed) {
    const Plan p = plan(rate);
    CHECK(p.rate_mid > 0 && p.rate_mid * p.M == rate * p.L && gcd(p.L, p.M) == 1);
    const int64_t L = p.L, M = p.M, C = (N - 1) / 2, P = phase_taps(N, L), H = history(N, L);
    CHECK(origin_ok(n_origin, p.rate_mid, L, M));
    std::vector<int64_t> ring((size_t)H, -1);            // the absolute index each cell of the history holds
    int64_t pushed = 0, k_done = k_origin(n_origin, L, M), k_model = k_done;
    CHECK(k_done * M == n_origin * L && mid_done(n_origin, n_origin, N, L, M) == k_done);
    const int64_t lens[6] = {1, M - 1 > 0 ? M - 1 : 1, M, 7919 < rate ? 7919 : 13, rate, 3};
    for (int step = 0; step < 300; step++) {
        seed = seed * 1664525u + 1013904223u;
        const int64_t n_new = lens[(seed >> 24) % 6];
        const int64_t n_start = n_origin + pushed, n_end = n_start + n_new;
        const int64_t k_new = mid_done(n_origin, n_end, N, L, M);
        // the brute-force model: walk k up while its last input exists (never skips, never repeats)
        if (n_new <= 8192) { while (last_input(k_model, N, L, M) < n_end) k_model++; }
        else k_model = k_new;
        CHECK(k_new == k_model && k_new >= k_done && k_new - k_done <= p.rate_mid);          // at most a second of intermediate samples
        CHECK(k_new == k_origin(n_origin, L, M) || last_input(k_new - 1, N, L, M) < n_end);
        CHECK(last_input(k_new, N, L, M) >= n_end);
        // what the kernel reads for the new samples, before the history is updated
        const int64_t p_last = pushed ? hist_pos(n_start - 1, n_origin, H) : 0;
        for (int64_t k = k_done; k < k_new; k += (k < k_done + 2 || k >= k_new - 3) ? 1 : (k_new - k_done) / 5 + 1) {
            const int64_t n1 = last_input(k, N, L, M), n0 = first_input(k, N, L, M), ph = phase(k, N, L, M);
            CHECK(n1 < n_end && n1 - n0 + 1 == P && ph >= 0 && ph < L && n1 * L + ph == k * M + C);
            // the true first input of the definition, ceil((t_k - N + 1) / L), is not before the kernel's
            const int64_t t = k * M + C, lo = t - N + 1, n_true = lo >= 0 ? (lo + L - 1) / L : -((-lo) / L);
            CHECK(n_true >= n0 && n_true <= n1);
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
        for (int64_t n = n_end - 1; n >= n_origin && n > n_end - 1 - H; n -= (n > n_end - 4 || n < n_end - H + 3) ? 1 : 89)
            CHECK(ring[(size_t)hist_pos(n, n_origin, H)] == n);
        // ... and the next sample not yet made needs nothing older than the history
        CHECK(first_input(k_done, N, L, M) > n_end - 1 - H);
    }
}

int main() {
    const int64_t rates[4] = {44100, 250000, 2048000, 10000000};
    const int64_t mids[4] = {48000, 48000, 192000, 48000}, ls[4] = {160, 24, 3, 3}, ms[4] = {147, 125, 32, 625};
    const int64_t taps[4] = {1007, 777, 179, 3873};
    const int64_t two32 = (int64_t)1 << 32;
    for (int i = 0; i < 4; i++) {
        const Plan p = plan(rates[i]);
        CHECK(p.rate_mid == mids[i] && p.L == ls[i] && p.M == ms[i]);
        const int64_t grid = origin_at(1, p);
        CHECK((grid * 12000) % (1008 * rates[i]) == 0);                                         // a whole number of 12 kHz tiles
        check_stream(rates[i], taps[i], 0, 1u + i);
        check_stream(rates[i], taps[i], grid * 3, 2u + i);
        check_stream(rates[i], taps[i], origin_at(two32 - 2 * grid, p) - grid, 3u + i);         // the pushes cross n = 2^32
        check_stream(rates[i], taps[i], origin_at((int64_t)1 << 50, p), 4u + i);
        // the origin rule
        CHECK(origin_ok(0, p.rate_mid, p.L, p.M) && origin_ok(grid, p.rate_mid, p.L, p.M) && !origin_ok(grid + 1, p.rate_mid, p.L, p.M));
        CHECK(!origin_ok(grid / 2 + 1, p.rate_mid, p.L, p.M) && !origin_ok(-grid, p.rate_mid, p.L, p.M) && !origin_ok(N_MAX + grid, p.rate_mid, p.L, p.M));
    }
    CHECK(origin_at(1, plan(10000000)) == 840000 && origin_at(1, plan(44100)) == 18522 && origin_at(1, plan(2048000)) == 172032);
    // more plans of the table, the refused rates, and rates another path takes
    CHECK(plan(16000).rate_mid == 48000 && plan(16000).L == 3 && plan(16000).M == 1 && plan(22050).L == 320 && plan(22050).M == 147);
    CHECK(plan(1000000).rate_mid == 48000 && plan(1000000).L == 6 && plan(20000000).rate_mid == 96000 && plan(20000000).M == 625);
    const int64_t refused[12] = {900001, 15999, 0, -44100, 129600001, 12000, 24000, 48000, 96000, 192000, 240000, 2400000};
    for (int64_t r : refused) CHECK(plan(r).rate_mid == 0 && plan(r).L == 0 && plan(r).M == 0);
    // every accepted rate of a sweep: the ratio is exact and in lowest terms, L within the limit, no other mid has a smaller L
    for (int64_t r = RATE_MIN; r <= RATE_MAX; r += (r < 3000000 ? 50 : 12500)) {
        const Plan p = plan(r);
        if (!p.rate_mid) continue;
        CHECK(p.L >= 1 && p.L <= MAX_L && p.rate_mid * p.M == r * p.L && gcd(p.L, p.M) == 1);
        for (int64_t mid = 48000; mid <= 192000; mid *= 2) CHECK(mid / gcd(r, mid) > p.L || (mid / gcd(r, mid) == p.L && mid <= p.rate_mid));
    }
    // the tiles of both regimes: at least one output, and the inputs under the tile fit the LDS image
    CHECK(lane_regime(1007, 160) && lane_regime(2421, 320) && lane_regime(777, 24) && lane_regime(179, 3) && !lane_regime(777, 6) && !lane_regime(3873, 3));
    CHECK(!lane_regime(5162, 160));                                                           // P = 33, but the table does not fit
    for (int i = 0; i < 4; i++) {
        const int64_t N = taps[i], L = ls[i], M = ms[i], P = phase_taps(N, L), t = tile_outputs(N, L, M);
        const int64_t span = last_input(1000 + t - 1, N, L, M) - last_input(1000, N, L, M);
        if (lane_regime(N, L)) CHECK(t >= 1 && t <= LANE_TILE && span + P <= LANE_SAMPLES && P * L <= LANE_TABLE);
        else CHECK(t >= 1 && t <= WAVE_TILE && span + PIECE <= WAVE_SAMPLES);
    }
    for (int64_t m = 1; m <= MAX_TAPS; m += 3)
        for (int64_t l = 1; l <= MAX_L; l += 29) {
            const int64_t a = tile_fit(LANE_SAMPLES, LANE_P, l, m, LANE_TILE), b = tile_fit(WAVE_SAMPLES, PIECE, l, m, WAVE_TILE);
            CHECK(a >= 1 && (a - 1) * m / l + 1 + LANE_P <= LANE_SAMPLES && b >= 1 && (b - 1) * m / l + 1 + PIECE <= WAVE_SAMPLES);
        }
    // the one-shot count: the samples a non-zero input can reach, capped, at least one
    CHECK(mid_count(0, 1007, 160, 147, 720000) == 1 && mid_count(661500, 1007, 160, 147, 720000) == 720000);
    for (int i = 0; i < 4; i++)
        for (int64_t n = 1; n < 3000; n += 7) {
            const int64_t N = taps[i], L = ls[i], M = ms[i], k = mid_count(n, N, L, M, (int64_t)1 << 40);
            // k - 1 still reaches the last input with its first tap h[0], k does not
            CHECK((k - 1) * M + (N - 1) / 2 - (N - 1) <= (n - 1) * L && k * M + (N - 1) / 2 - (N - 1) > (n - 1) * L);
        }
    printf("ddc rat ring arithmetic: %ld checked\n", checks);
    return 0;
}
