// Input sample kinds and formats: constexpr, so host and device alike, no runtime calls.  The ABI's eight
// kinds (include/ft8rx.h: FT8RX_DDC_* 0 .. 3, FT8RX_WIDE_* 16 .. 19) name six formats -- kinds 0 / 16 and 2 / 17 are the same bytes.
// An entry turns its kind into the format once, behind its argument checks (sample_fmt); kernels and stream state carry the format.
// pyft8_amd/kinds.py is the Python counterpart.
#pragma once
#include <stdint.h>
#include "../../include/ft8rx.h"

enum SampleFmt : int { SF_REAL_I16 = 0, SF_REAL_F32, SF_IQ_I16, SF_IQ_F32, SF_IQ_U8, SF_IQ_I8, SF_N };

// the table: components per sample (1 real, 2 an (I, Q) pair), bytes per component, integer or float
struct SampleFmtRow { int components, component_bytes; bool integer; };
constexpr SampleFmtRow sf_row(int fmt) {
    switch (fmt) {
        case SF_REAL_I16: return {1, 2, true};
        case SF_REAL_F32: return {1, 4, false};
        case SF_IQ_I16: return {2, 2, true};
        case SF_IQ_F32: return {2, 4, false};
        case SF_IQ_U8: return {2, 1, true};      // value 256 u - 32640 on the int16 scale (the blanker: 2 u - 255)
        default: return {2, 1, true};            // SF_IQ_I8: value 256 s
    }
}
constexpr int sf_components(int fmt) { return sf_row(fmt).components; }
constexpr int sf_component_bytes(int fmt) { return sf_row(fmt).component_bytes; }      // what the input blanker aligns to
constexpr int sf_sample_bytes(int fmt) { return sf_row(fmt).components * sf_row(fmt).component_bytes; }      // what ddc and the pre-stages align to
constexpr bool sf_is_iq(int fmt) { return sf_row(fmt).components == 2; }
constexpr bool sf_is_integer(int fmt) { return sf_row(fmt).integer; }
// a real input has half its power at the negative frequencies the filters remove: the gain that makes up for it
constexpr float sf_real_gain(int fmt) { return sf_is_iq(fmt) ? 1.0f : 2.0f; }

// the format of a public kind, or -1
constexpr int sample_fmt(int kind) {
    switch (kind) {
        case FT8RX_DDC_REAL_I16: case FT8RX_WIDE_REAL_I16: return SF_REAL_I16;
        case FT8RX_DDC_REAL_F32: return SF_REAL_F32;
        case FT8RX_DDC_IQ_I16: case FT8RX_WIDE_IQ_I16: return SF_IQ_I16;
        case FT8RX_DDC_IQ_F32: return SF_IQ_F32;
        case FT8RX_WIDE_IQ_U8: return SF_IQ_U8;
        case FT8RX_WIDE_IQ_I8: return SF_IQ_I8;
        default: return -1;
    }
}

// the kinds an entry family takes, bit k = kind k
constexpr uint32_t sf_kind_range(int lo, int hi) { return ((2u << hi) - 1u) & ~((1u << lo) - 1u); }
constexpr uint32_t SF_KINDS_DDC = sf_kind_range(FT8RX_DDC_REAL_I16, FT8RX_DDC_IQ_F32);
constexpr uint32_t SF_KINDS_WIDE = sf_kind_range(FT8RX_WIDE_REAL_I16, FT8RX_WIDE_IQ_I8);
constexpr uint32_t SF_KINDS_RAT = SF_KINDS_DDC | sf_kind_range(FT8RX_WIDE_IQ_U8, FT8RX_WIDE_IQ_I8);
constexpr uint32_t SF_KINDS_BLANK_IN = 1u << FT8RX_DDC_REAL_I16 | 1u << FT8RX_DDC_IQ_I16 | SF_KINDS_WIDE;
constexpr bool sf_kind_in(uint32_t kinds, int kind) { return kind >= 0 && kind < 32 && (kinds >> kind & 1u); }

static_assert(FT8RX_DDC_REAL_I16 == 0 && FT8RX_DDC_REAL_F32 == 1 && FT8RX_DDC_IQ_I16 == 2 && FT8RX_DDC_IQ_F32 == 3 && FT8RX_WIDE_REAL_I16 == 16 &&
              FT8RX_WIDE_IQ_I16 == 17 && FT8RX_WIDE_IQ_U8 == 18 && FT8RX_WIDE_IQ_I8 == 19, "include/ft8rx.h: the kinds");
static_assert(SF_KINDS_DDC == 0x0000000fu && SF_KINDS_WIDE == 0x000f0000u && SF_KINDS_RAT == 0x000c000fu && SF_KINDS_BLANK_IN == 0x000f0005u,
              "who takes which kind (the input blanker: the integer formats)");
