// ddc_frames_check.cpp -- stand-alone check of the argument checks of ft8rx_ddc_stream_frames (pyft8_amd/csrc/ddc_frames.hpp) and of the
// range rule it shares with the other gathers (ddc_ring.hpp: held) at both frame lengths, built with g++ -fsanitize=address,undefined
// and run on the CPU by tests/test_ft4_live.py.  It walks every gather a kernel thread would do for the ranges `held` admits through a
// model of one ring row and checks that each index it loads lies inside the row and holds the output asked for.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../pyft8_amd/csrc/ddc_frames.hpp"
#include "../pyft8_amd/csrc/ddc_ring.hpp"

using namespace ddcframes;

static long checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { fprintf(stderr, "ddc_frames_check: %s failed (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static bool says(Verdict v, int frame_len, int n_have, const int32_t* ch, int n_sel, int n_out, int max_frames, const char* word) {
    char msg[256];
    const int n = describe(msg, sizeof msg, "ft8rx_ddc_stream_frames", v, frame_len, n_have, ch, n_sel, n_out, max_frames);
    return n > 0 && n < (int)sizeof msg && strstr(msg, word) != nullptr && strstr(msg, "ft8rx_ddc_stream_frames: ") == msg;
}

static void check_arguments() {
    const int n_out = 3, mf = 5;
    const int32_t ok[5] = {2, 0, 1, 1, 1}, high[2] = {0, 3}, neg[3] = {1, -1, 9};
    for (int len : {FT8_LEN, FT4_LEN}) {
        CHECK(frame_len_ok(len));
        for (int n_have : {0, 1, 72000, len}) {
            CHECK(check(len, n_have, ok, 2, n_out, mf).bad == OK);
            CHECK(check(len, n_have, ok, 5, n_out, mf).bad == OK);            // repeats, n_sel above n_out up to max_frames
            CHECK(check(len, n_have, nullptr, 3, n_out, mf).bad == OK);       // NULL = 0 .. n_sel - 1
        }
        for (int n_have : {-1, len + 1, INT32_MAX, INT32_MIN}) {
            const Verdict v = check(len, n_have, ok, 2, n_out, mf);
            CHECK(v.bad == BAD_N_HAVE && says(v, len, n_have, ok, 2, n_out, mf, "n_have"));
        }
        for (int n_sel : {0, -1, mf + 1, INT32_MAX}) {                        // refused before the list is read
            const Verdict v = check(len, len, ok, n_sel, n_out, mf);
            CHECK(v.bad == BAD_N_SEL && says(v, len, len, ok, n_sel, n_out, mf, "n_sel"));
        }
        Verdict v = check(len, len, high, 2, n_out, mf);
        CHECK(v.bad == BAD_CHANNEL && v.at == 1 && says(v, len, len, high, 2, n_out, mf, "channel 3"));
        v = check(len, len, neg, 3, n_out, mf);
        CHECK(v.bad == BAD_CHANNEL && v.at == 1 && says(v, len, len, neg, 3, n_out, mf, "channel -1"));
        v = check(len, len, nullptr, 4, n_out, mf);                           // NULL with more frames than channels
        CHECK(v.bad == BAD_CHANNEL && v.at == 3 && says(v, len, len, nullptr, 4, n_out, mf, "channel 3"));
    }
    for (int len : {0, 1000, -90000, 90001, 179999, 360000, INT32_MAX}) {
        CHECK(!frame_len_ok(len));
        const Verdict v = check(len, 0, ok, 2, n_out, mf);                    // the first check: whatever else is wrong
        CHECK(v.bad == BAD_FRAME_LEN && says(v, len, 0, ok, 2, n_out, mf, "frame_len"));
        CHECK(check(len, -1, neg, 0, n_out, mf).bad == BAD_FRAME_LEN);
    }
    // the table: uploaded iff the list differs from the one it holds
    const int32_t t[3] = {2, 0, 1}, id[3] = {0, 1, 2};
    CHECK(!differs(t, 3, t, 3) && differs(t, 3, t, 2) && differs(t, 2, t, 3) && differs(t, 3, id, 3) && !differs(t, 3, ok, 3) && differs(nullptr, 0, t, 1));
    CHECK(!differs(id, 3, nullptr, 3) && differs(t, 3, nullptr, 3) && differs(id, 3, nullptr, 2));
}

// one ring row as the stream leaves it when outputs [m_origin, m_done) have been produced: cell m mod OUT_RING holds the newest m
static void check_gathers(int64_t m_origin, int64_t m_done) {
    using namespace ddcring;
    std::vector<int64_t> row((size_t)OUT_RING, INT64_MIN);
    for (int64_t m = (m_done - OUT_RING > m_origin ? m_done - OUT_RING : m_origin); m < m_done; m++) row[(size_t)out_pos(m)] = m;
    const int64_t oldest = m_done - OUT_RING > m_origin ? m_done - OUT_RING : m_origin;
    for (int len : {FT8_LEN, FT4_LEN}) {
        const int64_t firsts[] = {m_origin - 6001, m_origin - len - 5, m_origin, oldest - 1, oldest, oldest + 1, m_done - len, m_done - len - 1,
                                  m_done - 1001, m_done, 2 * (int64_t)FT8_LEN - 9999 + m_origin, -1, 1001};
        for (int64_t m_first : firsts)
            for (int n_have : {0, 1, 72000, len}) {
                const Range r = held(m_first, n_have, m_origin, m_done);
                const int64_t lo = m_first > m_origin ? m_first : m_origin, hi = m_first + n_have < m_done ? m_first + n_have : m_done;
                // refused iff an output it would read has been overwritten: the oldest one asked for is the first to go
                CHECK(r.ok == (hi <= lo || row[(size_t)out_pos(lo)] == lo));
                if (!r.ok) continue;
                for (int p = 0; p < len; p += (p < 3 || p > len - 3 || (p > n_have - 3 && p < n_have + 3)) ? 1 : 997) {   // the kernel's thread p
                    const int64_t m = m_first + p;
                    if (!(p < n_have && m >= m_origin && m < m_done)) continue;     // zero: no load
                    const int64_t at = m % OUT_RING;                                // m >= m_origin >= 0 here
                    CHECK(at >= 0 && at < OUT_RING && row[(size_t)at] == m);
                }
            }
    }
}

int main() {
    check_arguments();
    check_gathers(0, 33264);                                  // a young stream: nothing has wrapped
    check_gathers(0, 1008 * 755);                             // past two cycles: the ring has wrapped
    check_gathers(1008 * 5, 1008 * 5 + 1008 * 400);           // an origin off zero
    check_gathers(1008 * ((int64_t)1 << 30), 1008 * ((int64_t)1 << 30) + 1008 * 1000);
    printf("ddc frames arguments: %ld checks ok\n", checks);
    return 0;
}
