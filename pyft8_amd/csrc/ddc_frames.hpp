// ddc_frames.hpp -- the argument checks of ft8rx_ddc_stream_frames: which frame lengths the gather cuts, how
// much of a frame may be asked for, which channel lists it takes.  Pure host code beside ddc_ring.hpp, whose `held` says what the ring
// still has.  No HIP: compiles with plain g++ (tests/ddc_frames_check.cpp checks it under the host sanitizers).
#pragma once
#include <cstdint>
#include <cstdio>

namespace ddcframes {

constexpr int FT8_LEN = 180000;             // FT8RX_NSAMP: a 15-s frame
constexpr int FT4_LEN = 90000;              // FT8RX_FT4_NSAMP: a 7.5-s frame (ft8rx.hip holds both to the header by static_assert)

constexpr bool frame_len_ok(int frame_len) { return frame_len == FT8_LEN || frame_len == FT4_LEN; }

// what is wrong with a call, in the order the checks run; `at`: the index into channels of BAD_CHANNEL
enum Bad { OK = 0, BAD_FRAME_LEN, BAD_N_HAVE, BAD_N_SEL, BAD_CHANNEL };
struct Verdict { Bad bad; int at; };

// frame_len one of the two; 0 <= n_have <= frame_len; 1 <= n_sel <= max_frames; every channels[i] in [0, n_out), repeats allowed;
// channels NULL = 0 .. n_sel - 1, which must then all be channels
inline Verdict check(int frame_len, int n_have, const int32_t* channels, int n_sel, int n_out, int max_frames) {
    if (!frame_len_ok(frame_len)) return Verdict{BAD_FRAME_LEN, 0};
    if (n_have < 0 || n_have > frame_len) return Verdict{BAD_N_HAVE, 0};
    if (n_sel < 1 || n_sel > max_frames) return Verdict{BAD_N_SEL, 0};
    for (int i = 0; i < n_sel; i++) {
        const int32_t j = channels ? channels[i] : i;
        if (j < 0 || j >= n_out) return Verdict{BAD_CHANNEL, i};
    }
    return Verdict{OK, 0};
}

// the refusal, by name -> characters written (snprintf)
inline int describe(char* out, size_t cap, const char* who, Verdict v, int frame_len, int n_have, const int32_t* channels, int n_sel, int n_out,
                    int max_frames) {
    switch (v.bad) {
    case BAD_FRAME_LEN: return snprintf(out, cap, "%s: frame_len %d is neither %d (FT8) nor %d (FT4)", who, frame_len, FT8_LEN, FT4_LEN);
    case BAD_N_HAVE: return snprintf(out, cap, "%s: n_have %d outside [0, %d]", who, n_have, frame_len);
    case BAD_N_SEL: return snprintf(out, cap, "%s: n_sel %d outside [1, %d] (max_frames)", who, n_sel, max_frames);
    case BAD_CHANNEL: return snprintf(out, cap, "%s: channel %d (entry %d of the list) outside [0, %d)", who, (int)(channels ? channels[v.at] : v.at), v.at, n_out);
    default: return snprintf(out, cap, "%s: ok", who);
    }
}

// the list of a call (NULL = 0 .. n_sel - 1) against the one the device table holds: true = upload
inline bool differs(const int32_t* table, int n_table, const int32_t* channels, int n_sel) {
    if (n_table != n_sel) return true;
    for (int i = 0; i < n_sel; i++) if (table[i] != (channels ? channels[i] : i)) return true;
    return false;
}

}  // namespace ddcframes
