// ft4_sublist_check.cpp -- host sanitizer target for ft8rx_ft4_subtraction_list's body (hostmsg::ft4_subtraction_list, DESIGN.md section
// 19.6).  TEST INFRASTRUCTURE.  Compiles pyft8_amd/csrc/host_messages.hpp on its own (g++ -fsanitize=address,undefined; no HIP) and
// drives the list with hand-made and random records: exact expectations for order, repeats and the have-list, then random frames
// with counts beyond the row, caps of one signal, tweaks at the ends of their range and have-counts beyond their row -- every output
// array is allocated to its exact size, so a stray access is the sanitizer's to report.
//   g++ -std=c++17 -fsanitize=address,undefined -pthread -o ft4_sublist_check tests/ft4_sublist_check.cpp && ./ft4_sublist_check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include <set>
#include <utility>
#include <vector>
#include "../include/ft8rx.h"
#include "../pyft8_amd/csrc/ft8_tables.h"
#include "../pyft8_amd/csrc/host_messages.hpp"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "ft4 subtraction list: %s fails (line %d)\n", #x, __LINE__); return 1; } } while (0)

static ft8rx_record rec_of(uint64_t lo, uint64_t hi, int f0, int h0, int tt, int ft, int ipass, float score, int status) {
    ft8rx_record r; memset(&r, 0, sizeof(r));
    r.msg_lo = lo; r.msg_hi = hi; r.f0_idx = (int16_t)f0; r.h0_idx = (int16_t)h0; r.ttweak = (int8_t)tt; r.ftweak = (int8_t)ft;
    r.ipass = (uint8_t)ipass; r.score = r.grid_sd = r.fine_sd = score; r.status = (uint8_t)status;
    return r;
}

int main() {
    static_assert(sizeof(ft8rx_ft4_subsig) == 120, "the record is 120 bytes");
    long checked = 0;
    {   // the hand-made frame: BP decodes before OSD's, each in score order; a repeat; an undecoded slot; a word the frame has
        const int MC = 8;
        std::vector<ft8rx_record> R(MC);
        R[0] = rec_of(11, 0, 100, 40, 1, -2, 4, 900.f, FT8RX_ST_DECODED);
        R[1] = rec_of(22, 1, 300, 41, 0, 0, 5, 800.f, FT8RX_ST_DECODED);
        R[2] = rec_of(11, 0, 101, 40, -4, 2, 4, 700.f, FT8RX_ST_DECODED);
        R[3] = rec_of(99, 0, 50, -5, 3, 1, 4, 650.f, FT8RX_ST_EXHAUSTED);
        R[4] = rec_of(33, 2, 200, 60, 2, -1, 4, 600.f, FT8RX_ST_DECODED);
        R[5] = rec_of(44, 0, 566, 167, 4, 2, 4, 500.f, FT8RX_ST_DECODED);
        R[6] = rec_of(55, 0, 0, -1024, -4, -2, 4, 400.f, FT8RX_ST_DECODED);        // fq = -2: left out
        int32_t cnt = 7, sc = -1;
        std::vector<ft8rx_ft4_subsig> S(4);
        CHECK(hostmsg::ft4_subtraction_list(R.data(), &cnt, MC, 1, nullptr, nullptr, nullptr, 0, S.data(), 4, &sc) == 4 && sc == 4);
        uint8_t t[105];
        const uint64_t want_lo[4] = {11, 33, 44, 22}, want_hi[4] = {0, 2, 0, 1};
        for (int i = 0; i < 4; i++) { hostmsg::encode_tones_ft4(want_lo[i], want_hi[i], t); CHECK(memcmp(t, S[i].tones, 105) == 0); }
        CHECK(S[0].start == 144 * 40 + 36 && S[0].fq == 398 && S[2].start == 144 * 167 + 144 && S[2].fq == 2266 && S[3].start == 144 * 41);
        for (int i = 0; i < 4; i++) for (int k = 0; k < 7; k++) CHECK(S[i].pad[k] == 0);
        const uint64_t hl[2] = {33, 11}, hh[2] = {2, 0}; const int32_t hc = 2;
        CHECK(hostmsg::ft4_subtraction_list(R.data(), &cnt, MC, 1, hl, hh, &hc, 2, S.data(), 4, &sc) == 2 && sc == 2);
        hostmsg::encode_tones_ft4(44, 0, t); CHECK(memcmp(t, S[0].tones, 105) == 0);
        hostmsg::encode_tones_ft4(22, 1, t); CHECK(memcmp(t, S[1].tones, 105) == 0);
        CHECK(hostmsg::ft4_subtraction_list(R.data(), &cnt, MC, 1, nullptr, nullptr, nullptr, 0, S.data(), 1, &sc) == 1 && sc == 1);     // the cap
        CHECK(hostmsg::ft4_subtraction_list(nullptr, &cnt, MC, 1, nullptr, nullptr, nullptr, 0, S.data(), 1, &sc) == -1);
        CHECK(hostmsg::ft4_subtraction_list(R.data(), &cnt, MC, 1, nullptr, nullptr, nullptr, 0, S.data(), 0, &sc) == -1);
        checked += 7;
    }
    std::mt19937_64 rng(4242);
    for (int round = 0; round < 400; round++) {
        const int B = 1 + (int)(rng() % 5), MC = 1 + (int)(rng() % 40), MS = 1 + (int)(rng() % 12), MH = (int)(rng() % 6);
        std::vector<ft8rx_record> R((size_t)B * MC);
        std::vector<int32_t> cnt(B), sc(B), hc(B);
        std::vector<uint64_t> hl((size_t)B * (MH ? MH : 1)), hh(hl.size());
        for (auto& r : R) {
            const uint64_t lo = rng() % 12, hi = rng() % 2;                 // few words: many repeats
            const int ipass = (rng() % 4) ? 4 + (int)(rng() % 2) : (int)(rng() % 9), status = (rng() % 3) ? FT8RX_ST_DECODED : (int)(rng() % 6);
            r = rec_of(lo, hi, (int)(rng() % 1300) - 100, (int)(rng() % 2100) - 1050, (int)(rng() % 256) - 128, (int)(rng() % 256) - 128,
                       ipass, (float)(rng() % 1000), status);
        }
        for (int f = 0; f < B; f++) { cnt[f] = (int)(rng() % (MC + 20)) - 5; hc[f] = (int)(rng() % (MH + 4)) - 1; }
        for (size_t i = 0; i < hl.size(); i++) { hl[i] = rng() % 12; hh[i] = rng() % 2; }
        std::vector<ft8rx_ft4_subsig> S((size_t)B * MS);
        const bool with = MH > 0 && (round & 1);
        const int most = hostmsg::ft4_subtraction_list(R.data(), cnt.data(), MC, B, with ? hl.data() : nullptr, with ? hh.data() : nullptr,
                                                       with ? hc.data() : nullptr, MH, S.data(), MS, sc.data());
        CHECK(most >= 0 && most <= MS);
        for (int f = 0; f < B; f++) {
            CHECK(sc[f] >= 0 && sc[f] <= most);
            std::set<std::vector<uint8_t>> seen;
            const int nh = !with ? 0 : hc[f] < 0 ? 0 : hc[f] > MH ? MH : hc[f];
            uint8_t t[105];
            for (int j = 0; j < nh; j++) { hostmsg::encode_tones_ft4(hl[(size_t)f * MH + j], hh[(size_t)f * MH + j], t); seen.insert(std::vector<uint8_t>(t, t + 105)); }
            for (int i = 0; i < sc[f]; i++) {
                const ft8rx_ft4_subsig& g = S[(size_t)f * MS + i];
                CHECK(g.fq >= 0 && g.fq < 4608);
                CHECK(seen.insert(std::vector<uint8_t>(g.tones, g.tones + 105)).second);       // no repeat, nothing the frame has
                for (int k = 0; k < 105; k++) CHECK(g.tones[k] < 4);
                checked++;
            }
        }
    }
    printf("ft4 subtraction list: %ld checked\n", checked);
    return 0;
}
