// Stand-alone check of pyft8_amd/csrc/blank_in_ring.hpp (the index arithmetic of the input-rate noise blanker)
// against brute force, for small B, G, R, origins and chunkings.  tests/test_blank_in.py builds it with
// g++ -fsanitize=address,undefined and runs it: every work-buffer position is used as a real array index here.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../pyft8_amd/csrc/blank_in_ring.hpp"

static long long g_checks = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { fprintf(stderr, "blank_in_ring_check: %s failed (line %d)\n", #c, __LINE__); exit(1); } } while (0)

// the finality rule, sample by sample: n is final once every block up to (n + G + R) / B + 2 is complete
static int64_t released_brute(int64_t n_origin, int64_t n_end, int64_t B, int64_t G, int64_t R) {
    int64_t n = n_origin;
    while (n < n_end && ((n + G + R) / B + 3) * B <= n_end) n++;
    return n;
}

// one stream in the chunks `cut` (repeated as needed), n_total samples, then finish: what the plans say against a model that keeps
// every sample's absolute index in the work buffers
static void run_stream(int64_t B, int64_t G, int64_t R, int64_t n_origin, int64_t n_total, const std::vector<int64_t>& cut, bool finish_with_last) {
    int64_t max_push = 1;
    for (int64_t c : cut) if (c > max_push) max_push = c;
    const int64_t cap = blankin::capacity(B, G, R, max_push);
    std::vector<int64_t> work[2] = {std::vector<int64_t>((size_t)cap, -1), std::vector<int64_t>((size_t)cap, -1)};
    int cur = 0;
    int64_t base = n_origin / B * B, pushed = 0, lv_done = n_origin / B, hb_done = n_origin / B, rel = n_origin, prev_rel = n_origin;
    size_t k = 0;
    bool finished = false;
    while (!finished) {
        int64_t n_new = cut[k++ % cut.size()];
        if (n_new > n_total - pushed) n_new = n_total - pushed;
        const bool last = pushed + n_new == n_total;
        const bool fin = last && finish_with_last;
        const int64_t n_start = n_origin + pushed;
        const blankin::Plan p = blankin::plan(n_origin, n_start, n_new, fin, B, G, R);
        // the release: brute force, monotone, never past n_end, contiguous with the last push
        CHECK(p.n_end == n_start + n_new && p.g0 == rel && p.g0 == blankin::released(n_origin, n_start, B, G, R));
        CHECK(blankin::released(n_origin, p.n_end, B, G, R) == released_brute(n_origin, p.n_end, B, G, R));
        CHECK(p.g1 >= p.g0 && p.g1 <= p.n_end && (fin ? p.g1 == p.n_end : p.g1 == released_brute(n_origin, p.n_end, B, G, R)));
        CHECK(p.g1 - p.g0 <= n_new + B || fin);
        CHECK(p.n_end - p.g1 <= 3 * B + G + R || p.g1 == n_origin);                   // the latency bound
        // the buffers: the leftover moves to the other one, the chunk follows it, every index inside the capacity
        CHECK(p.base % B == 0 && p.base <= p.g0 && p.g0 - p.base < B && p.left_n == n_start - p.g0 && p.left_n < 3 * B + G + R + (p.g0 == n_origin ? B : 0));
        std::vector<int64_t>& nw = work[cur ^ 1];
        const std::vector<int64_t>& old = work[cur];
        for (int64_t i = 0; i < p.left_n; i++) nw.at((size_t)(p.g0 - p.base + i)) = old.at((size_t)(p.g0 - base + i));
        for (int64_t i = 0; i < n_new; i++) nw.at((size_t)(n_start - p.base + i)) = n_start + i;
        for (int64_t n = p.g0; n < p.n_end; n++) CHECK(nw.at((size_t)(n - p.base)) == n);
        CHECK(p.n_end - p.base <= cap);
        // levels: contiguous, complete blocks only (the tail block with finish), each read inside the buffer
        CHECK(p.lv0 == lv_done && p.lv1 >= p.lv0 && p.b_have == p.lv1 && p.b_first == n_origin / B);
        CHECK(fin ? p.lv1 == (p.n_end + B - 1) / B : p.lv1 == (p.n_end / B > p.b_first ? p.n_end / B : p.b_first));
        for (int64_t b = p.lv0; b < p.lv1; b++)
            for (int64_t n = b * B; n < (b + 1) * B; n++)
                if (n >= n_origin && n < p.n_end) CHECK(nw.at((size_t)(n - p.base)) == n);
        // hits: contiguous, m of b + 2 exists (or lies outside the finished stream), the samples still raw: not released before
        CHECK(p.hb0 == hb_done && p.hb1 >= p.hb0 && p.m_hi == p.hb1 * B);
        for (int64_t b = p.hb0; b < p.hb1; b++) {
            CHECK(fin || b + 2 < p.b_have);
            for (int64_t n = b * B; n < (b + 1) * B; n++)
                if (n >= n_origin && n < p.n_end) { CHECK(n >= p.g0 && p.g0 >= prev_rel); CHECK(nw.at((size_t)(n - p.base)) == n); }
        }
        // the gate: every hit within G + R of a released sample is known
        if (p.g1 > p.g0) CHECK(fin || p.g1 - 1 + G + R < p.m_hi);
        CHECK(p.hb0 * B >= p.base || p.hb0 == p.hb1);
        prev_rel = p.g0; rel = p.g1; lv_done = p.lv1; hb_done = p.hb1; base = p.base; cur ^= 1; pushed += n_new;
        if (last) {
            if (!fin) {                                                              // finish as a push of its own, with no samples
                const blankin::Plan q = blankin::plan(n_origin, n_origin + pushed, 0, true, B, G, R);
                CHECK(q.g0 == rel && q.g1 == n_origin + pushed && q.lv0 == lv_done && q.hb0 == hb_done && q.hb1 == q.lv1 && q.left_n == q.n_end - q.g0);
                CHECK(q.n_end - q.base <= cap);
            }
            finished = true;
        }
    }
}

int main() {
    for (int64_t B : {8, 16, 32})
        for (int64_t G : {0, 1, 3})
            for (int64_t R : {0, 2, 5})
                for (int64_t n_origin : {(int64_t)0, (int64_t)1, B - 1, B, 5 * B + 3, ((int64_t)1 << 40) + 7}) {
                    // released: monotone in n_end, never past it, the brute-force rule
                    int64_t last = n_origin;
                    for (int64_t n_end = n_origin; n_end < n_origin + 9 * B; n_end++) {
                        const int64_t r = blankin::released(n_origin, n_end, B, G, R);
                        CHECK(r >= last && r <= n_end && r >= n_origin && r == released_brute(n_origin, n_end, B, G, R));
                        last = r;
                    }
                    const int64_t n_total = 7 * B + 5;
                    const std::vector<std::vector<int64_t>> cuts = {{1}, {B - 1}, {B}, {B + 1}, {3 * B + G + R}, {1, B - 1, 3, B + 1, 2 * B + 5, 7, B}, {n_total}};
                    for (const auto& cut : cuts)
                        for (bool fin : {false, true}) run_stream(B, G, R, n_origin, n_total, cut, fin);
                    run_stream(B, G, R, n_origin, 3, {2}, true);                      // shorter than a block
                    run_stream(B, G, R, n_origin, 2 * B, {B}, false);                 // whole blocks only
                }
    printf("blank in ring arithmetic: %lld checks passed\n", g_checks);
    return 0;
}
