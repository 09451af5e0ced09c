// Stand-alone check of pyft8_amd/csrc/pan_ring.hpp (the index arithmetic of the panorama) against brute force,
// for small N, A, ring sizes, origins and chunkings.  tests/test_pan.py builds it with g++ -fsanitize=address,undefined and runs it:
// every work-buffer position and ring slot is used as a real array index here.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../pyft8_amd/csrc/pan_ring.hpp"

static long long g_checks = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { fprintf(stderr, "pan_ring_check: %s failed (line %d)\n", #c, __LINE__); exit(1); } } while (0)

// row r exists once all its samples [r A N, (r + 1) A N) lie in [n_origin, n_end): the first such row, and the first that does not yet
static int64_t r_first_brute(int64_t n_origin, int64_t N, int64_t A) {
    int64_t r = n_origin / (A * N) > 2 ? n_origin / (A * N) - 2 : 0;      // (a start below the answer: the search is the rule)
    while (r * A * N < n_origin) r++;
    return r;
}
static int64_t rows_done_brute(int64_t n_origin, int64_t n_end, int64_t N, int64_t A) {
    int64_t r = r_first_brute(n_origin, N, A);
    while ((r + 1) * A * N <= n_end) r++;
    return r;
}

// one stream in the chunks `cut` (repeated as needed), n_total samples: what the plans say against a model that keeps every sample's
// absolute index in the work buffer and the leftover, and every window's index in the ring slot of its row
static void run_stream(int64_t N, int64_t A, int64_t n_rows, int64_t tile_cap, int64_t n_origin, int64_t n_total, const std::vector<int64_t>& cut) {
    int64_t max_push = 1;
    for (int64_t c : cut) if (c > max_push) max_push = c;
    std::vector<int64_t> work((size_t)panring::capacity(N, max_push), -1), left((size_t)N, -1);
    const int64_t slots = panring::slots(n_rows), tile = panring::tile_windows(tile_cap, n_rows, A);
    CHECK(tile >= 1 && tile <= tile_cap);
    // per slot: the row it holds and how many of its windows have been added, in order
    std::vector<int64_t> slot_row((size_t)slots, -1), slot_cnt((size_t)slots, 0);
    const int64_t rf = r_first_brute(n_origin, N, A);
    CHECK(panring::r_first(n_origin, N, A) == rf && panring::w_first(n_origin, N, A) == rf * A);
    int64_t pushed = 0, w_next = rf * A, left_n = 0, r_done = rf;
    size_t k = 0;
    while (pushed < n_total) {
        int64_t n_new = cut[k++ % cut.size()];
        if (n_new > n_total - pushed) n_new = n_total - pushed;
        const int64_t n_start = n_origin + pushed;
        const panring::Plan p = panring::plan(n_origin, n_start, n_new, N, A);
        CHECK(p.n_end == n_start + n_new && p.w0 == w_next && p.w1 >= p.w0 && p.left_n == left_n && p.left_n < N);
        CHECK(p.w1 == (p.n_end / N > rf * A ? p.n_end / N : rf * A));
        CHECK(p.base == n_start - p.left_n && p.chunk_at == p.left_n);
        // the buffer: the leftover to the front, the chunk behind it
        for (int64_t i = 0; i < p.left_n; i++) work.at((size_t)i) = left.at((size_t)i);
        for (int64_t i = 0; i < n_new; i++) work.at((size_t)(p.chunk_at + i)) = n_start + i;
        for (int64_t i = 0; i < p.left_n + n_new; i++) CHECK(work.at((size_t)i) == p.base + i);
        // every sample of every window of this push is where the plan says
        for (int64_t w = p.w0; w < p.w1; w++)
            for (int64_t i = 0; i < N; i++) {
                const int64_t at = p.first_at + (w - p.w0) * N + i;
                CHECK(work.at((size_t)at) == w * N + i && w * N + i >= n_origin && w * N + i < p.n_end);
            }
        // the tiles: the rows a tile touches have distinct slots; a row starts from zero at its first window and counts up in order
        for (int64_t t = p.w0; t < p.w1; t += tile) {
            const int64_t t1 = t + tile < p.w1 ? t + tile : p.w1, ra = t / A, rb = (t1 - 1) / A;
            CHECK(rb - ra + 1 <= slots);
            for (int64_t r = ra; r <= rb; r++) {
                const int64_t lo = r * A > t ? r * A : t, hi = (r + 1) * A < t1 ? (r + 1) * A : t1;
                const size_t s = (size_t)(r % slots);
                if (lo == r * A) { slot_row.at(s) = r; slot_cnt.at(s) = 0; }
                CHECK(slot_row.at(s) == r && slot_cnt.at(s) == lo - r * A);
                slot_cnt.at(s) += hi - lo;
            }
        }
        // rows: brute force; the held rows are whole and in their slots
        CHECK(p.r0 == r_done && p.r1 == rows_done_brute(n_origin, p.n_end, N, A) && p.r1 == panring::rows_done(n_origin, p.n_end, N, A));
        const panring::Held h = panring::held(n_origin, p.n_end, N, A, n_rows);
        CHECK(h.r_hi == p.r1 && h.r_lo >= rf && h.r_hi - h.r_lo <= n_rows && (h.r_lo == rf || h.r_hi - h.r_lo == n_rows));
        for (int64_t r = h.r_lo; r < h.r_hi; r++) CHECK(slot_row.at((size_t)(r % slots)) == r && slot_cnt.at((size_t)(r % slots)) == A);
        // what the next push needs goes to the leftover
        CHECK(p.keep_n < N && p.keep_n >= 0 && p.keep_at >= 0 && p.keep_at + p.keep_n == p.left_n + n_new);
        for (int64_t i = 0; i < p.keep_n; i++) left.at((size_t)i) = work.at((size_t)(p.keep_at + i));
        for (int64_t i = 0; i < p.keep_n; i++) CHECK(left.at((size_t)i) == p.n_end - p.keep_n + i);
        CHECK(p.keep_n == 0 || p.n_end - p.keep_n == p.w1 * N);
        left_n = p.keep_n; w_next = p.w1; r_done = p.r1; pushed += n_new;
    }
}

int main() {
    for (int64_t N : {4, 8})
        for (int64_t A : {1, 3, 5})
            for (int64_t n_rows : {1, 2, 7})
                for (int64_t tile_cap : {1, 4, 1000})
                    for (int64_t n_origin : {(int64_t)0, (int64_t)1, N - 1, N, N * A, N * A + 1, 5 * N * A + 3, ((int64_t)1 << 40) + 7}) {
                        int64_t last = panring::rows_done(n_origin, n_origin, N, A);
                        for (int64_t n_end = n_origin; n_end < n_origin + 4 * N * A + 3; n_end++) {      // monotone, the brute-force rule
                            const int64_t r = panring::rows_done(n_origin, n_end, N, A);
                            CHECK(r >= last && r == rows_done_brute(n_origin, n_end, N, A) && panring::windows_done(n_origin, n_end, N, A) >= r * A);
                            last = r;
                        }
                        const int64_t n_total = 11 * N * A + 5;
                        const std::vector<std::vector<int64_t>> cuts = {{1}, {N - 1}, {N}, {N + 1}, {A * N - 1}, {A * N + 1}, {1, N - 1, N, N + 1, A * N - 1, A * N + 1, 7}, {n_total}};
                        for (const auto& cut : cuts) run_stream(N, A, n_rows, tile_cap, n_origin, n_total, cut);
                        run_stream(N, A, n_rows, tile_cap, n_origin, 3, {2});                 // shorter than a window
                    }
    printf("pan ring arithmetic: %lld checks passed\n", g_checks);
    return 0;
}
