// ap_patterns.hpp -- the ipass-7 a-priori patterns of ft8rx_set_ap_calls (the operator's own call MY, the DX station's call DX)
// Part of libft8rx.so; included by ft8rx.hip before bp.hpp / osd.hpp, whose AP7 twins read it.  The kernels are in ap_calls.hpp.
#ifndef FT8RX_AP_PATTERNS_HPP
#define FT8RX_AP_PATTERNS_HPP

// Patterns, numbered as the record's `ap` field (0..4 are the reference's, llr.hpp: ap_value):
//   5 MY ???       6 MY DX ???     7 CQ DX ???          partial: known LLR positions forced to +-5, then BP_B, then OSD
//   8 MY DX RRR    9 MY DX 73     10 MY DX RR73         full: a codeword test against the hard decisions
// Bits are LLR positions (= transmitted order: message bit 76 - i at position i; the i3 = 1 layout c28 0-27, r1 28, c28 29-56, r1 57,
// R1 58, g15 59-73, i3 74-76), bit i of a pattern at word i >> 6, bit i & 63.
#define FT8RX_AP_FIRST 5
#define FT8RX_AP_N 6
struct ApCalls {
    int32_t np;                       // enabled patterns (0 = the setting is off: nothing of ipass 7 is launched)
    int32_t max_hd;                   // acceptance gate: distance of the accepted codeword to the un-overridden hard decisions
    int32_t pat[FT8RX_AP_N];          // the enabled patterns, ascending
    uint64_t val[FT8RX_AP_N][3];      // [pattern - 5]: known bit values (full patterns: the whole 174-bit codeword)
    uint64_t msk[FT8RX_AP_N][3];      // [pattern - 5]: which positions are known
    uint64_t lo[FT8RX_AP_N], hi[FT8RX_AP_N];     // the full patterns' 77-bit words (record layout: bit 76 = first transmitted bit)
};

// the LLR of position i under pattern ap (5..7): +-5 where the pattern knows the bit (as ap_value does), v elsewhere
FT8_DEV float ap7_value(const ApCalls* __restrict__ a, int ap, int i, float v) {
    const int k = ap - FT8RX_AP_FIRST, w = i >> 6, b = i & 63;
    if (!((a->msk[k][w] >> b) & 1ull)) return v;
    return ((a->val[k][w] >> b) & 1ull) ? 5.0f : -5.0f;
}

#endif
