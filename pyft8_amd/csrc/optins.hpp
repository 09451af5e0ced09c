// optins.hpp -- which opt-in steps refuse which: the relation the setters of ft8rx.hip and ft8rx_decode_messages enforce, stated
// once.  No HIP: compiles with plain g++ (tests/host_asan_driver.cpp checks it; pyft8_amd/optins.py is its twin for the Python
// surface, and tests/test_gpu_optins.py ties the two together).  Adding an opt-in: DESIGN.md section 15.
#pragma once

namespace optins {

// the six handle settings, then the C-side consumer of a batch that cannot carry some of them
enum Id { PACKED, MSG_TYPES, AP_CALLS, RECALL, WEAK, REPORTS, N_SETTINGS, DECODE_MESSAGES = N_SETTINGS, N_ROWS };
constexpr unsigned bit(Id i) { return 1u << i; }

struct Row { const char* name; unsigned excludes; };      // the name refusals use, and the settings this one cannot run with
// Among the six settings the relation is symmetric: msg_types, ap_calls, recall and weak exclude each other except ap_calls +
// recall (ipass 7 and ipass 8 run one after the other), the packed output carries none of them, reports only lack a place in it.
constexpr Row TABLE[N_ROWS] = {
    {"the packed output (ft8rx_set_packed_output)", bit(MSG_TYPES) | bit(AP_CALLS) | bit(RECALL) | bit(WEAK) | bit(REPORTS)},
    {"msg_types != 0",                              bit(PACKED) | bit(AP_CALLS) | bit(RECALL) | bit(WEAK)},
    {"ft8rx_set_ap_calls",                          bit(PACKED) | bit(MSG_TYPES) | bit(WEAK)},
    {"ft8rx_set_recall",                            bit(PACKED) | bit(MSG_TYPES) | bit(WEAK)},
    {"ft8rx_set_weak",                              bit(PACKED) | bit(MSG_TYPES) | bit(AP_CALLS) | bit(RECALL)},
    {"ft8rx_set_reports",                           bit(PACKED)},
    {"ft8rx_decode_messages",                       bit(MSG_TYPES) | bit(RECALL)},      // ft8rx_message rows hold neither
};

// FT4 decoding (ft8rx_ft4_*), a consumer row of its own: its ladder is BP and OSD on the demodulator's LLRs with
// the msg_types mask, nothing else.  (TABLE's rows are the ones tests/host_asan_driver.cpp holds to its literal truth table.)
constexpr Row FT4_ROW = {"FT4 decoding (ft8rx_ft4_decode_batch)", bit(PACKED) | bit(AP_CALLS) | bit(RECALL) | bit(WEAK) | bit(REPORTS)};

// the first setting, in table order, that is active and that the row cannot run with; -1 = none
constexpr int conflict(unsigned active, const Row& row) {
    const unsigned hit = active & row.excludes;
    for (int i = 0; i < N_SETTINGS; i++) if (hit & (1u << i)) return i;
    return -1;
}
inline int conflict(unsigned active, Id asked) { return conflict(active, TABLE[asked]); }

}  // namespace optins
