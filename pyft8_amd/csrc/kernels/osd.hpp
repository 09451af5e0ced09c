// osd.hpp -- ordered-statistics decoding (decoders.py:223-272)
// Part of libft8rx.so; included by ft8rx.hip (single translation unit: the kernels share __constant__/__device__ tables).
#ifndef FT8RX_OSD_HPP
#define FT8RX_OSD_HPP

// ------------------------------------------------------------------------------------ OSD (decoders.py:223-272)
// One wavefront per attempt (osd_attempt: osd_load, osd_order, osd_eliminate, osd_flip_table, osd_syndromes, osd_trials), three ideas:
//   1. reliability order = np.argsort(-abs(llr)) as the reference's numpy (2.2.6 on AVX-512: x86-simd-sort) orders it, equal keys
//      included: that library's 256-wire compare-exchange network run on (key, index) pairs held in registers, exchanged by DPP /
//      ds_swizzle / ds_bpermute; a vector with a NaN takes the library's other path, std::sort, on one lane (rare);
//   2. most-reliable-basis Gauss-Jordan over GF(2) with the generator held COLUMN-wise: lane l owns columns l, 64+l, 128+l
//      of G0 (91 row bits each, 3 x u32).  A visited column is broadcast to scalar registers; "independent of the accepted
//      columns" is then a scalar test (any 1 in an unlocked row), the pivot row a scalar find-first-set, and the elimination
//      one masked XOR per owned column -- no ballots, no cross-lane shuffles, nothing on the dependent chain but readlanes;
//   3. trials: CRC-14 is linear, so each trial's syndrome is the XOR of the precomputed syndromes of the order-0 codeword
//      and of its flip rows; a lane tests one trial with three 16-bit LDS reads.  Only zero-syndrome trials (2^-14 of them)
//      rebuild the codeword, run the validity predicate and log the reference's unpack() call.
// The trial list (order 0, single flips, the reference's restricted double flips, then the build's order-3 extension) is a
// table built by the host from the configuration, in the reference's trial order (decoders.py:248-272).
// Timing-only builds (-DOSD_TIMING, tools/osd_timing.py): lane 0 of every attempt adds the shader cycles between consecutive marks OT(i) to
// g_osd_t[]; a phase with a mark inside takes the attempt's clock `ot` (an empty struct in the product).  Never defined in the product.
#ifdef OSD_TIMING
__device__ unsigned long long g_osd_t[32768][10];       // per block: plain adds by lane 0 of its one wave, summed by the host (no atomics in the timed code)
struct OsdClock { unsigned long long prev = __builtin_readcyclecounter(); };
#define OT(i) do { const unsigned long long ot_now = __builtin_readcyclecounter(); if (lane == 0) g_osd_t[blockIdx.x & 32767][i] += ot_now - ot.prev; ot.prev = __builtin_readcyclecounter(); } while (0)
#define OT_FLUSH do { if (lane == 0) g_osd_t[blockIdx.x & 32767][9] += 1ull; } while (0)
#else
struct OsdClock {};
#define OT(i) do { } while (0)
#define OT_FLUSH do { } while (0)
#endif
// ---- np.argsort's compare-exchange network (oracle/ft8_oracle.c: ft8o_argsort_f32 has the derivation and the library references).
// 256 wires = 32 registers of 8 lanes in the library; here wire w = 64 q + lane sits in register q of the lane.  Every stage pairs wire w
// with w ^ M, the LOWER wire keeps the smaller key, and equal keys never move (the library moves an index only when min / max did not
// return the lane's own key).  Stage masks: 1 3 1 7 2 1 | 15 4 2 1 | 31 8 4 2 1 | 63 16 8 4 2 1 | 127 32 16 8 4 2 1 | 255 64 32 16 8 4 2 1.
// osd_px<M>: the value of lane ^ M, M < 64: quad permutes / row mirrors (DPP) for 1, 2, 3, 7, 15, a row rotate for 8, ds_swizzle (crossbar only,
// no address register) for 4, 16, 31, ds_bpermute for 32 and 63.
template <int M> FT8_DEV uint32_t osd_px(uint32_t v, int lane) {
    if (M == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);          // quad_perm:[1,0,3,2]
    if (M == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);          // quad_perm:[2,3,0,1]
    if (M == 3) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x1B, 0xf, 0xf, false);          // quad_perm:[3,2,1,0]
    if (M == 7) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false);         // row_half_mirror
    if (M == 15) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false);        // row_mirror
    if (M == 8) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);         // row_ror:8
    if (M == 4 || M == 16 || M == 31) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1f | (M << 10));   // bit mode: lane ^ M within 32
    return __shfl(v, lane ^ M);
}
// One stage between lanes M apart on NQ registers of (key, index) pairs.  The sort is a fifth of the attempt's vector instructions and the
// kernel is bound by their number, so a register-stage is written out: both orders of the pair (min, max), the lane's side picked with a
// constant lane mask (a scalar operand), "the key changed" = "take the partner's index" -- 5 vector instructions where the compare-and-
// select form compiled to ~14.  For the strides a DPP control reaches (1, 2, 3, 7, 15, 8) the partner is read as a DPP operand of v_min /
// v_max / v_cndmask themselves (inline assembly: the compiler only fuses a DPP move into a single user).  Hazards the assembler does not
// see inside an asm block: VALU writes VCC -> VALU reads VCC needs two wait states on gfx950 (the s_nop below); a DPP read of a VGPR needs
// two wait states after the VALU write -- the blocks of the other register sets (or of the previous stage) lie in between.
#define OSD_LOWMASK(top) ((top) == 1 ? 0x5555555555555555ull : (top) == 2 ? 0x3333333333333333ull : (top) == 4 ? 0x0F0F0F0F0F0F0F0Full : \
                          (top) == 8 ? 0x00FF00FF00FF00FFull : (top) == 16 ? 0x0000FFFF0000FFFFull : 0x00000000FFFFFFFFull)
#define OSD_DPP_STAGE(CTRL)                                                                                                          \
    asm volatile("v_min_u32_dpp %[mn], %[hk], %[hk] " CTRL " row_mask:0xf bank_mask:0xf\n\t"                                         \
                 "v_max_u32_dpp %[mx], %[hk], %[hk] " CTRL " row_mask:0xf bank_mask:0xf\n\t"                                         \
                 "v_cndmask_b32 %[mn], %[mx], %[mn], %[low]\n\t"                                                                    \
                 "v_cmp_eq_u32 vcc, %[mn], %[hk]\n\t"                                                                                \
                 "s_nop 1\n\t"                                                                                                       \
                 "v_cndmask_b32_dpp %[ix], %[ix], %[ix], vcc " CTRL " row_mask:0xf bank_mask:0xf\n\t"                                \
                 : [mn] "=&v"(mn), [mx] "=&v"(mx), [ix] "+v"(ix[q]) : [hk] "v"(hk[q]), [low] "s"(low) : "vcc");
template <int M, int NQ> FT8_DEV void osd_stage(uint32_t* hk, uint32_t* ix, int lane) {
    constexpr int top = M >= 32 ? 32 : M >= 16 ? 16 : M >= 8 ? 8 : M >= 4 ? 4 : M >= 2 ? 2 : 1;      // highest bit of M: clear on the lower wire
    const uint64_t low = OSD_LOWMASK(top);                     // lanes that hold the lower wire of their pair
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        uint32_t mn, mx;
        if constexpr (M == 1) { OSD_DPP_STAGE("quad_perm:[1,0,3,2]") }
        else if constexpr (M == 2) { OSD_DPP_STAGE("quad_perm:[2,3,0,1]") }
        else if constexpr (M == 3) { OSD_DPP_STAGE("quad_perm:[3,2,1,0]") }
        else if constexpr (M == 7) { OSD_DPP_STAGE("row_half_mirror") }
        else if constexpr (M == 15) { OSD_DPP_STAGE("row_mirror") }
        else if constexpr (M == 8) { OSD_DPP_STAGE("row_ror:8") }
        else {
            const uint32_t pk = osd_px<M>(hk[q], lane), pi = osd_px<M>(ix[q], lane);
            mn = pk < hk[q] ? pk : hk[q]; mx = pk < hk[q] ? hk[q] : pk;
            asm("v_cndmask_b32 %0, %1, %0, %2" : "+v"(mn) : "v"(mx), "s"(low));      // lower wire: the minimum
            ix[q] = (mn == hk[q]) ? ix[q] : pi;
        }
        hk[q] = mn;
    }
}
#undef OSD_DPP_STAGE
template <int NQ> FT8_DEV void osd_stages_421(uint32_t* hk, uint32_t* ix, int lane) {
    osd_stage<4, NQ>(hk, ix, lane); osd_stage<2, NQ>(hk, ix, lane); osd_stage<1, NQ>(hk, ix, lane);
}
// register a (lower wires) against register b, same lane (reversed = false) or lane 63 - l (reversed = true: the first stage of a merge)
template <bool REV> FT8_DEV void osd_stage_regs(uint32_t& ka, uint32_t& ia, uint32_t& kb, uint32_t& ib, int lane) {
    const uint32_t pkb = REV ? __shfl(kb, 63 - lane) : kb, pib = REV ? __shfl(ib, 63 - lane) : ib;      // what a's lane faces
    const uint32_t pka = REV ? __shfl(ka, 63 - lane) : ka, pia = REV ? __shfl(ia, 63 - lane) : ia;      // what b's lane faces
    const uint32_t na = pkb < ka ? pkb : ka, nb = pka > kb ? pka : kb;                                   // a keeps the minimum, b the maximum
    ia = (na == ka) ? ia : pib; ib = (nb == kb) ? ib : pia;
    ka = na; kb = nb;
}
// ---- the library's path for a vector that contains a NaN (std_argsort_withnan): libstdc++'s std::sort of the index array with the
// comparator "both not NaN: a < b; a NaN: false; else true" on the keys -|llr|.  One lane, in LDS; rare (a NaN-poisoned BP output,
// decoders.py:143-147).  Function for function as in oracle/ft8_oracle.c (std_sort_withnan), with the recursion on the right part
// turned into an explicit stack (the parts are disjoint, their order does not matter).
#define FT8_HD __host__ __device__ inline
FT8_HD bool osd_nl(const float* x, int a, int b) {
    const float xa = x[a], xb = x[b];
    if (xa == xa && xb == xb) return fabsf(xa) > fabsf(xb);             // -|xa| < -|xb|
    return xa == xa;                                                    // a NaN: false; a number against a NaN: true
}
FT8_HD void osd_ss_linear_insert(const float* x, int* a, int last) {
    const int val = a[last]; int next = last - 1;
    while (osd_nl(x, val, a[next])) { a[last] = a[next]; last = next; next--; }
    a[last] = val;
}
FT8_HD void osd_ss_insertion(const float* x, int* a, int first, int last) {
    for (int i = first + 1; i < last; i++) {
        if (osd_nl(x, a[i], a[first])) { const int val = a[i]; for (int j = i; j > first; j--) a[j] = a[j - 1]; a[first] = val; }
        else osd_ss_linear_insert(x, a, i);
    }
}
FT8_HD void osd_ss_adjust_heap(const float* x, int* a, int first, int hole, int len, int value) {
    const int top = hole; int child = hole;
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);
        if (osd_nl(x, a[first + child], a[first + child - 1])) child--;
        a[first + hole] = a[first + child]; hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) { child = 2 * (child + 1); a[first + hole] = a[first + child - 1]; hole = child - 1; }
    int parent = (hole - 1) / 2;                                        // __push_heap
    while (hole > top && osd_nl(x, a[first + parent], value)) { a[first + hole] = a[first + parent]; hole = parent; parent = (hole - 1) / 2; }
    a[first + hole] = value;
}
FT8_HD void osd_std_sort_withnan(const float* x, int* a, int* stack /* [3 * 20] */) {
    const int n = 174;
    for (int i = 0; i < n; i++) a[i] = i;
    int sp = 0;
    stack[0] = 0; stack[1] = n; stack[2] = 2 * 7; sp = 1;              // depth limit 2 * floor(lg 174)
    while (sp > 0) {
        sp--;
        int first = stack[3 * sp], last = stack[3 * sp + 1], depth = stack[3 * sp + 2];
        while (last - first > 16) {
            if (depth == 0) {                                           // heapsort (__partial_sort(first, last, last))
                const int len = last - first;
                for (int parent = (len - 2) / 2; parent >= 0; parent--) osd_ss_adjust_heap(x, a, first, parent, len, a[first + parent]);
                while (last - first > 1) { last--; const int v = a[last]; a[last] = a[first]; osd_ss_adjust_heap(x, a, first, 0, last - first, v); }
                break;
            }
            depth--;
            {   // __move_median_to_first(first, first + 1, mid, last - 1)
                const int p = first + 1, q = first + (last - first) / 2, r = last - 1;
                int pick;
                if (osd_nl(x, a[p], a[q])) pick = osd_nl(x, a[q], a[r]) ? q : (osd_nl(x, a[p], a[r]) ? r : p);
                else pick = osd_nl(x, a[p], a[r]) ? p : (osd_nl(x, a[q], a[r]) ? r : q);
                const int t = a[first]; a[first] = a[pick]; a[pick] = t;
            }
            int lo = first + 1, hi = last;                              // __unguarded_partition(first + 1, last, pivot = *first)
            for (;;) {
                while (osd_nl(x, a[lo], a[first])) lo++;
                hi--;
                while (osd_nl(x, a[first], a[hi])) hi--;
                if (!(lo < hi)) break;
                const int t = a[lo]; a[lo] = a[hi]; a[hi] = t;
                lo++;
            }
            stack[3 * sp] = lo; stack[3 * sp + 1] = last; stack[3 * sp + 2] = depth; sp++;      // the right part, later
            last = lo;
        }
    }
    osd_ss_insertion(x, a, 0, 16);                                      // __final_insertion_sort, n > 16
    for (int i = 16; i < n; i++) osd_ss_linear_insert(x, a, i);
}

#undef FT8_HD
// the order std::sort leaves an ALL-NaN vector in (the comparator is then always false: a fixed permutation; ft8rx_create fills it by
// running the routine above on the host): the common NaN case -- a NaN-poisoned BP output is NaN everywhere -- stays in the main kernel
__device__ uint8_t d_NANPERM[192];

#define OSD_MAXFLIP 91            /* flip rows kept per attempt = all 91 basis positions (decoders.py:244-246 takes any count up to the basis size) */
#define OSD_FLIPS_A 62            /* flips 0..61: one bit each in the column's 64-bit word (bit 63 = order-0 codeword bit); flips 62..90: a second, 32-bit word
                                     that only exists for attempts with more than 62 flip rows (the reference's own callers use 30 / 40) */
#define OSD_MAXTRIALS 16384       /* trial index must fit the 16-bit seq of the event log */
#define OSD_NONE 0xFFu            /* "no flip" in a packed trial entry (i | j << 8 | k << 16) */

// CRC syndrome of codeword bit v alone (v < 77: message bit, 77..90: the CRC field bit itself), bit-sliced: d_SYNM[k][w] bit b = bit k
// of the syndrome of codeword bit 32 w + b.  Constant address space: wave-uniform reads become scalar loads (a uniform lookup in a
// 16-bit __device__ table is a broadcast vector load -- 91 of them per attempt kept the texture-address path busy, profiles/archive/r02_notes.md)
__device__ __constant__ uint32_t d_SYNM[14][3];
__device__ uint32_t d_G0T[192][3];       // column v of G0 = [I | A^T]: row bits 0..31, 32..63, 64..90 (columns >= 174 are zero)

// What a kernel of the family hands every attempt: its arguments (saved, attB, max_hd, nanlist, mt: k_osd* / k_osd_nan* only; apc: k_osd_ap*)
struct OsdArgs {
    const float* llr_in; const float* saved; const Att* attB; ft8rx_record* rec; const int32_t* ncand; Att* attO;
    ft8rx_event* ev; int32_t* evcount; const uint32_t* trials; int ntr, nflip, max_hd, sh; WorkList nanlist; unsigned mt; const ApCalls* apc;
};

// The attempt's LDS (one wave per block, declared once in osd_attempt).  `work` changes hands; a block barrier separates the owners:
//   osd_order<NANV = true>   ordl()  [174] the order std::sort leaves, then from ordl() + 176 its range stack [60]
//   osd_eliminate            posrow() [91] position of systematic column v
//   osd_flip_table onwards   ftabB() [192] per column: bit i - 62 = flip i covers it (62 <= i < 91; WIDE only), and frow() [OSD_MAXFLIP] the
//                            pivot row of flip i
struct OsdLds {
    float llr[176];
    uint64_t work[256];
    uint64_t ftab[192];                       // per column (natural order): bit i = flip i covers it (i < 62), bit 63 = order-0 codeword bit
    uint32_t hmw[3];                          // rows whose accepted column has hard decision 1
    uint16_t fsyn[OSD_MAXFLIP + 2];           // [i] flip i, [OSD_MAXFLIP] = 0 ("no flip"), [OSD_MAXFLIP + 1] order-0 codeword
    FT8_DEV int* ordl() { return reinterpret_cast<int*>(work); }
    FT8_DEV int* posrow() { return reinterpret_cast<int*>(work); }
    FT8_DEV uint32_t* ftabB() { return reinterpret_cast<uint32_t*>(work); }
    FT8_DEV int* frow() { return reinterpret_cast<int*>(work) + 192; }
};
static_assert(176 + 3 * 20 <= 512 && 192 + OSD_MAXFLIP <= 512 && sizeof(OsdLds) <= 4496, "the overlays fit the 512 words of work[]; 4.5 KB per block");

// ---- the input.  mode 0: pipeline (bid = candidate * 10 + slot 0..9); mode 2: raw vectors (bid = vector); AP7: bid = candidate << 4 |
// pattern (5..7), the fine LLRs with the pattern's known bits.  Fills llr[]; `vec` is the attempt's slot in attO, `hsrc` the vector
// whose hard decisions an accepted codeword's distance is measured to (AP7: the un-overridden fine LLRs).  go = false: nothing to do.
struct OsdInput { bool go; int slot; size_t vec; const float* hsrc; };
template <bool AP7>
FT8_DEV OsdInput osd_load(OsdLds& L, int lane, int mode, int bid, const OsdArgs& a) {
    OsdInput in = {true, 0, (size_t)bid, L.llr};
    if constexpr (AP7) {
        in.slot = bid & 15; const size_t c = (size_t)(bid >> 4);
        in.hsrc = a.llr_in + c * 174;
        const float v0 = in.hsrc[lane], v1 = in.hsrc[64 + lane], v2 = in.hsrc[128 + (lane < 46 ? lane : 0)];
        L.llr[lane] = ap7_value(a.apc, in.slot, lane, v0); L.llr[64 + lane] = ap7_value(a.apc, in.slot, 64 + lane, v1);
        if (lane < 46) L.llr[128 + lane] = ap7_value(a.apc, in.slot, 128 + lane, v2);
        in.vec = c * 10 + (in.slot - 5);
    } else if (mode == 0) {
        const int slot = in.slot = bid % 10; const int c = bid / 10;
        in.go = false;
        if ((c & ((1 << a.sh) - 1)) >= a.ncand[c >> a.sh]) return in;
        if (a.rec[c].status != FT8RX_ST_ACTIVE) return in;
        if (slot >= 5 && !a.attB[(size_t)c * 5 + (slot - 5)].has_out) { if (lane == 0) { Att u; memset(&u, 0, sizeof(u)); u.n_its = -1; a.attO[(size_t)c * 10 + slot] = u; } return in; }
        in.go = true;
        // slots 0..4: the fine LLRs with the AP override, slots 5..9: the saved BP outputs; three loads in flight either way
        const float* src = slot < 5 ? a.llr_in + (size_t)c * 174 : a.saved + ((size_t)c * 5 + (slot - 5)) * 174;
        const int apx = slot < 5 ? slot : 0;                                   // ap_value(0, ...) is the identity
        const float v0 = src[lane], v1 = src[64 + lane], v2 = src[128 + (lane < 46 ? lane : 0)];
        L.llr[lane] = ap_value(apx, lane, v0); L.llr[64 + lane] = ap_value(apx, 64 + lane, v1);
        if (lane < 46) L.llr[128 + lane] = ap_value(apx, 128 + lane, v2);
        in.vec = (size_t)c * 10 + slot;
    } else {
        for (int i = lane; i < 174; i += 64) L.llr[i] = a.llr_in[in.vec * 174 + i];
    }
    __syncthreads();
    return in;
}

// ---- reliability order: np.argsort(-abs(llr)) as the reference's numpy orders it (decoders.py:226; the network above) -> ix[q] = the
// column at reliability position 64 q + lane.  Keys: the magnitude bits, inverted so that an ascending unsigned sort is |llr|
// descending; padding wires (174 .. 255) hold the largest key.  Register 3 would be all padding and stays all padding up to the last
// merge: every stage that involves it is resolved by hand.
// NANV: the kernel of the attempts whose vector holds a NaN (k_osd_nan*).  The library sorts such a vector with std::sort -- a serial
// algorithm, run by one lane, whose code costs the main kernel 8 VGPRs and a scratch frame if it lives there: the main kernels
// (NANV = false) only append such an attempt to `nanlist` and leave (false: the attempt ends here); the NaN kernels stride over that
// list (almost always empty).  k_osd_ap passes no list: a vector with a NaN is skipped on purpose, the attempt keeps the undecoded result
// k_bp_ap wrote.  Fine LLRs can hold NaNs (a NaN sd passes the sd gate), and a word forced onto such a candidate has nothing to be
// measured against.
template <bool NANV>
FT8_DEV bool osd_order(OsdLds& L, int lane, int bid, const WorkList& nanlist, uint32_t* ix, OsdClock& ot) {
    uint32_t hk[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int i = lane + 64 * q;
        const uint32_t mag = __float_as_uint(L.llr[i < 174 ? i : 0]) & 0x7fffffffu;
        hk[q] = (i < 174) ? 0xFFFFFFFEu - mag : 0xFFFFFFFFu;
        ix[q] = (i < 174) ? (uint32_t)i : 0u;
    }
    const uint64_t nan0 = __ballot(hk[0] < 0x807FFFFEu), nan1 = __ballot(hk[1] < 0x807FFFFEu), nan2 = __ballot(lane < 46 && hk[2] < 0x807FFFFEu);      // magnitude bits above infinity's
    const bool any_nan = (nan0 | nan1 | nan2) != 0, all_nan = (nan0 & nan1) == ~0ull && nan2 == (1ull << 46) - 1;
    OT(0);
    if (NANV) {                                               // the library's std::sort path, one lane (k_osd_nan)
        if (!any_nan || all_nan) return false;                // (never: the list only holds vectors with some, not only, NaNs)
        int* ordl = L.ordl();
        if (lane == 0) osd_std_sort_withnan(L.llr, ordl, ordl + 176);
        __syncthreads();
        ix[0] = (uint32_t)ordl[lane]; ix[1] = (uint32_t)ordl[64 + lane]; ix[2] = (uint32_t)ordl[128 + (lane < 46 ? lane : 0)];
        __syncthreads();
    } else if (all_nan) {                                     // std::sort of 174 NaNs: a fixed permutation
        ix[0] = d_NANPERM[lane]; ix[1] = d_NANPERM[64 + lane]; ix[2] = d_NANPERM[128 + lane];
    } else if (any_nan) {                                     // wave-uniform, rare: left to the NaN kernel
        if (lane == 0) work_push(nanlist, bid);
        return false;
    } else {
        // inside the registers: each register's 64 wires sorted (8 library registers), three at a time
        osd_stage<1, 3>(hk, ix, lane); osd_stage<3, 3>(hk, ix, lane); osd_stage<1, 3>(hk, ix, lane);
        osd_stage<7, 3>(hk, ix, lane); osd_stage<2, 3>(hk, ix, lane); osd_stage<1, 3>(hk, ix, lane);
        osd_stage<15, 3>(hk, ix, lane); osd_stages_421<3>(hk, ix, lane);
        osd_stage<31, 3>(hk, ix, lane); osd_stage<8, 3>(hk, ix, lane); osd_stages_421<3>(hk, ix, lane);
        osd_stage<63, 3>(hk, ix, lane); osd_stage<16, 3>(hk, ix, lane); osd_stage<8, 3>(hk, ix, lane); osd_stages_421<3>(hk, ix, lane);
        // merge of 16 library registers: wires 0..63 against 127..64 reversed (registers 0 / 1); registers 2 / 3: 3 is padding, 2 is
        // sorted and stays as it is through this whole merge
        osd_stage_regs<true>(hk[0], ix[0], hk[1], ix[1], lane);
        osd_stage<32, 2>(hk, ix, lane); osd_stage<16, 2>(hk, ix, lane); osd_stage<8, 2>(hk, ix, lane); osd_stages_421<2>(hk, ix, lane);
        // merge of 32: w against 255 - w (register 1 against register 2 reversed; register 0 faces padding), then registers 0 / 1 lane
        // by lane (2 faces padding), then the lane strides on all three
        osd_stage_regs<true>(hk[1], ix[1], hk[2], ix[2], lane);
        osd_stage_regs<false>(hk[0], ix[0], hk[1], ix[1], lane);
        osd_stage<32, 3>(hk, ix, lane); osd_stage<16, 3>(hk, ix, lane); osd_stage<8, 3>(hk, ix, lane); osd_stages_421<3>(hk, ix, lane);
    }
    return true;
}

// hard decisions of v[0 .. 173] in natural order, as three lane masks (the distance test of the trials' slow path)
struct OsdHard { uint64_t w0, w1, w2; };
FT8_DEV OsdHard osd_hard(const float* v, int lane) {
    return {__ballot(v[lane] > 0.0f), __ballot(v[64 + lane] > 0.0f), __ballot(lane < 46 && v[128 + (lane < 46 ? lane : 0)] > 0.0f)};
}

// ---- the most reliable basis.  Lane l of register set s holds what belongs to reliability position 64 s + l: the column of the reduced
// generator (xs0, xs1, xs2 = rows 0..31, 32..63, 64..90), "in the basis" (bit l of acc<s>: its column is then a unit vector), hard decision (hs<s>)
struct OsdBasis {
    uint32_t x00, x01, x02, x10, x11, x12, x20, x21, x22;
    uint64_t acc0, acc1, acc2;
    bool hs0, hs1, hs2;
};
// Gauss-Jordan over GF(2), generator held column-wise in SORTED order: lane l of register set s owns the column at
// reliability position 64 s + l (91 row bits: rows 0..63 as two u32, rows 64..90 in a third).  A row is "locked" once it has
// been made the unit row of an accepted column.  Visiting position ic (decoders.py:228-242 visits the columns in this order):
// the column is broadcast to scalar registers (3 readlanes of a statically known register -- the loop is split per register
// set); it is independent of the accepted columns iff it has a 1 in an unlocked row; its lowest such row r becomes the pivot
// (which row is picked does not change the result: the reduced matrix of a given basis is unique up to row labels, and the
// codeword / flip rows below are label-free); clearing the column's other 1s = adding row r to those rows = XORing (column
// minus bit r) into every column that has a 1 in row r.  A column that already is a unit vector needs no update at all (the
// still untouched systematic columns: about 40 % of the basis).  The scalar pipe issues one instruction per cycle per CU and
// is this kernel's bottleneck (profiles/archive/r02_notes.md), so the bookkeeping is kept to lock words and one accepted-position bit
// per step; everything that can wait (hard-decision mask, flip rows, syndromes) is done afterwards on the vector side.
FT8_DEV OsdBasis osd_eliminate(OsdLds& L, int lane, const uint32_t* ix, OsdClock& ot) {
    const int ord0 = (int)ix[0], ord1 = (int)ix[1], ord2 = (lane < 46) ? (int)ix[2] : 0;
    const bool has2 = lane < 46;
    uint32_t x00 = d_G0T[ord0][0], x01 = d_G0T[ord0][1], x02 = d_G0T[ord0][2];
    uint32_t x10 = d_G0T[ord1][0], x11 = d_G0T[ord1][1], x12 = d_G0T[ord1][2];
    uint32_t x20 = has2 ? d_G0T[ord2][0] : 0u, x21 = has2 ? d_G0T[ord2][1] : 0u, x22 = has2 ? d_G0T[ord2][2] : 0u;
    const bool hs0 = L.llr[ord0] > 0.0f, hs1 = L.llr[ord1] > 0.0f, hs2 = has2 && L.llr[ord2] > 0.0f;
    uint64_t acc0 = 0, acc1 = 0, acc2 = 0;             // accepted positions per register set
    int k = 0;
    // SYSTEMATIC COLUMNS ARE NOT VISITED.  Column v < 91 of G0 = [I | A^T] is the unit vector e_v, and it stays e_v until some
    // pivot takes row v (an elimination only touches columns with a 1 in the pivot row).  Reached with row v free it is accepted with
    // pivot v and changes nothing -- about half of the ~105 visited positions, each costing the full broadcast / test / lock round on
    // the scalar pipe, the kernel's bottleneck.  So: the systematic columns at positions < OSD_TRIV ("trivial") are accepted without a
    // visit, the loop walks the other positions only (a bit mask per register set, find-first-set), and the free choice of the pivot
    // row keeps them trivial: a visited column takes its pivot among the rows that do NOT belong to a trivial column (lockU = locked or
    // reserved) -- there are as many such rows as pivots needed, up to the few positions the basis ends before or after OSD_TRIV.
    // Only a column with no 1 left there STEALS: among its 1s in rows of trivial columns positioned AFTER it (a trivial column before
    // it has been accepted: its row is locked) it takes the lowest, and the robbed column -- no longer a unit vector -- goes back
    // onto the visit list.  The basis is complete when visited accepts + trivial positions passed reach 91 (tcN: the number of
    // trivial positions before a lane).  Same information set as the plain loop, position for position: tests/test_osd_info_set.py (this rule as
    // plain Python on orders with many, few and no steals) and test_osd_steals_exact (tests/test_gpu_parity.py: the same vectors through the kernel).
#define OSD_TRIV 96
    int* posrow = L.posrow();
    if (ord0 < 91) posrow[ord0] = lane;
    if (ord1 < 91) posrow[ord1] = 64 + lane;
    if (has2 && ord2 < 91) posrow[ord2] = 128 + lane;
    uint64_t triv0 = __ballot(ord0 < 91), triv1 = __ballot(ord1 < 91 && lane < OSD_TRIV - 64);
    int tc0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(triv0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)triv0, 0));
    int tc1 = __popcll(triv0) + __builtin_amdgcn_mbcnt_hi((uint32_t)(triv1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)triv1, 0));
    int ntriv = __popcll(triv0) + __popcll(triv1);
    __syncthreads();
    // rows reserved for trivial columns: bit r = systematic column r sits at a position < OSD_TRIV
    const uint64_t u01 = __ballot(posrow[lane] < OSD_TRIV);
    const uint32_t u2 = (uint32_t)__ballot(lane < 27 && posrow[64 + (lane < 27 ? lane : 0)] < OSD_TRIV);
    uint64_t vis0 = ~triv0, vis1 = ~triv1, vis2 = (1ull << 46) - 1;
    // One visit = one straight path, integers only on the scalar side (a boolean that lives across a branch becomes a lane mask and
    // drags selects onto the vector pipe).  Both pipes are close to their ceilings in this loop -- eight waves x (SALU + VALU per visit)
    // x 4 cycles is what a round of visits takes (profiles/r05_notes.md) -- so the visit is counted in instructions:
    //   * every visit marks its position accepted and counts it (ACC, k) without a test; the rare paths take that back: the steal
    //     branch only replaces the eligible rows (a01, a2), and a dependent column (no eligible row at all) clears its mark, uncounts
    //     itself and runs the rest with an empty pivot b = 0 -- no column "has a 1 in row b", the update mask is zero everywhere;
    //   * the locked rows exist once (lockU = pivots taken + rows reserved for trivial columns); the steal branch works out which
    //     reserved rows are up for grabs from posrow and the trivial masks;
    //   * the update: "a 1 in the pivot row" as an all-ones / zero mask, then (mask & m) ^ x per word -- one v_bitop3 each on gfx950;
    //   * columns at positions already passed never change again (an accepted one is a unit vector at a locked row, a rejected one has
    //     all its 1s in rows that were locked when it was visited, and a pivot row is an unlocked row): while register set 1 is
    //     walked, set 0 is left alone; while set 2 is walked, sets 0 and 1.
    // TCV: trivial positions before a lane of this register set; BASE: its first position; VIS: its visit mask.  When the basis is
    // complete every visit mask is emptied, which ends this loop and skips the ones that follow.
    // (the accept step exists three times, once per word the pivot row can lie in -- the lowest eligible row is looked for word by word
    // anyway -- so that "a 1 in the pivot row" is ONE v_bfe_i32 of a statically known register: 4 vector instructions per register set)
#define OSD_UPD(XW, X0, X1, X2) { const uint32_t mk = (uint32_t)__builtin_amdgcn_sbfe((int)(XW), bp, 1u); X0 ^= mk & m0; X1 ^= mk & m1; X2 ^= mk & m2; }
#define OSD_STEP(XA, XB, XC, ACC, VIS, TCV, BASE, UPD0, UPD1, UPD2)                                                                \
    while (VIS != 0) {                                                                                                             \
        const int il = __builtin_ctzll(VIS);                                                                                       \
        if (k + __builtin_amdgcn_readlane(TCV, il) >= 91) { vis0 = 0; vis1 = 0; vis2 = 0; continue; }      /* completed by a trivial column before this one */ \
        const uint64_t bit = 1ull << il;                                                                                           \
        VIS &= ~bit; ACC |= bit; k++;                                                                                              \
        const uint32_t c0 = __builtin_amdgcn_readlane(XA, il), c1 = __builtin_amdgcn_readlane(XB, il), c2 = __builtin_amdgcn_readlane(XC, il); \
        uint32_t a0 = c0 & ~lockU0, a1 = c1 & ~lockU1, a2 = c2 & ~lockU2;                                                          \
        if (__builtin_expect(!(a0 | a1 | a2), 0)) {            /* rare: nothing outside the locked and reserved rows -- steal, or dependent */ \
            const int p = (BASE) + il;                                                                                             \
            /* rows of columns that are still trivial and come after this position (lane = row; a robbed column's row is a pivot's) */ \
            const int pa = posrow[lane], pb = posrow[64 + (lane < 27 ? lane : 0)];                                                 \
            const bool ta = pa > p && pa < OSD_TRIV && (((pa < 64 ? triv0 >> pa : triv1 >> (pa - 64)) & 1ull) != 0);               \
            const bool tb = lane < 27 && pb > p && pb < OSD_TRIV && (((pb < 64 ? triv0 >> pb : triv1 >> (pb - 64)) & 1ull) != 0);  \
            const uint64_t s01 = (((uint64_t)c1 << 32) | c0) & __ballot(ta);                                                       \
            a0 = (uint32_t)s01; a1 = (uint32_t)(s01 >> 32); a2 = c2 & (uint32_t)__ballot(tb);                                      \
            if (a0 | a1 | a2) {                                                                                                    \
                const int r = s01 ? __builtin_ctzll(s01) : 64 + __builtin_ctz(a2);                                                 \
                const int q = __builtin_amdgcn_readfirstlane(posrow[r]);   /* the robbed trivial column: visited like any other from now on */ \
                if (q < 64) { triv0 &= ~(1ull << q); vis0 |= 1ull << q; tc0 -= (lane > q) ? 1 : 0; tc1 -= 1; }                    \
                else { triv1 &= ~(1ull << (q - 64)); vis1 |= 1ull << (q - 64); tc1 -= (lane > q - 64) ? 1 : 0; }                   \
                ntriv--;                                                                                                           \
            } else { ACC &= ~bit; k--; }                       /* dependent on the accepted columns */                             \
        }                                                                                                                          \
        asm volatile("" : "+s"(a2));                           /* opaque: nothing about the branch above is threaded into the code below */ \
        /* the accept step: pivot = the lowest eligible row, clear the column's other 1s everywhere, lock the row */                \
        if (a0) {                                                                                                                  \
            const uint32_t b = a0 & (0u - a0), bp = __builtin_ctz(a0), m0 = c0 & ~b, m1 = c1, m2 = c2;                             \
            UPD0                                                                                                                   \
            lockU0 |= b;                                                                                                           \
        } else if (a1) {                                                                                                           \
            const uint32_t b = a1 & (0u - a1), bp = __builtin_ctz(a1), m0 = c0, m1 = c1 & ~b, m2 = c2;                             \
            UPD1                                                                                                                   \
            lockU1 |= b;                                                                                                           \
        } else {                                               /* (a2 = 0: a dependent column -- bit 31 of the third word is never set: mask 0, no row locked) */ \
            const uint32_t b = a2 & (0u - a2), bp = __builtin_ctz(a2 | 0x80000000u), m0 = c0, m1 = c1, m2 = c2 & ~b;               \
            UPD2                                                                                                                   \
            lockU2 |= b;                                                                                                           \
        }                                                                                                                          \
    }
    // locked by a pivot, or reserved for a trivial column (rows 91 .. 95 do not exist)
    uint32_t lockU0 = (uint32_t)u01, lockU1 = (uint32_t)(u01 >> 32), lockU2 = ~((1u << 27) - 1u) | u2;
    OT(2);
    OSD_STEP(x00, x01, x02, acc0, vis0, tc0, 0,
             OSD_UPD(x00, x00, x01, x02) OSD_UPD(x10, x10, x11, x12) OSD_UPD(x20, x20, x21, x22),
             OSD_UPD(x01, x00, x01, x02) OSD_UPD(x11, x10, x11, x12) OSD_UPD(x21, x20, x21, x22),
             OSD_UPD(x02, x00, x01, x02) OSD_UPD(x12, x10, x11, x12) OSD_UPD(x22, x20, x21, x22))
    OSD_STEP(x10, x11, x12, acc1, vis1, tc1, 64,
             OSD_UPD(x10, x10, x11, x12) OSD_UPD(x20, x20, x21, x22),
             OSD_UPD(x11, x10, x11, x12) OSD_UPD(x21, x20, x21, x22),
             OSD_UPD(x12, x10, x11, x12) OSD_UPD(x22, x20, x21, x22))
    {
        int tc2 = ntriv;                                      // every trivial position lies before register set 2
        OSD_STEP(x20, x21, x22, acc2, vis2, tc2, 128, OSD_UPD(x20, x20, x21, x22), OSD_UPD(x21, x20, x21, x22), OSD_UPD(x22, x20, x21, x22))
    }
#undef OSD_STEP
#undef OSD_UPD
    // the trivial columns of the basis: the first 91 - k of them
    acc0 |= __ballot(((triv0 >> lane) & 1ull) && tc0 < 91 - k);
    acc1 |= __ballot(((triv1 >> lane) & 1ull) && tc1 < 91 - k);
    __syncthreads();                                          // posrow is done with: the flip rows overlay it
    return {x00, x01, x02, x10, x11, x12, x20, x21, x22, acc0, acc1, acc2, hs0, hs1, hs2};
}

// ---- the flip table: which columns (natural order) each flip row and the order-0 codeword cover -> ftab[], ftabB() (WIDE), frow()
template <bool WIDE>
FT8_DEV void osd_flip_table(OsdLds& L, int lane, const uint32_t* ix, const OsdBasis& b, int nflip, OsdClock& ot) {
    const int nflipA = WIDE ? OSD_FLIPS_A : nflip;          // WIDE: nflip > OSD_FLIPS_A (the launcher picks the kernel)
    const bool has2 = lane < 46;
    const int ord0 = (int)ix[0], ord1 = (int)ix[1], ord2 = has2 ? (int)ix[2] : 0;
    // Acceptance order = position order, so the accepted column at position p is the kk-th accepted one with kk = number of accepted
    // positions before p.
    const bool in0 = (b.acc0 >> lane) & 1ull, in1 = (b.acc1 >> lane) & 1ull, in2 = (b.acc2 >> lane) & 1ull;
    const int n0 = __popcll(b.acc0), n1 = __popcll(b.acc1);
    const int kk0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(b.acc0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b.acc0, 0));
    const int kk1 = n0 + __builtin_amdgcn_mbcnt_hi((uint32_t)(b.acc1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b.acc1, 0));
    const int kk2 = n0 + n1 + __builtin_amdgcn_mbcnt_hi((uint32_t)(b.acc2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b.acc2, 0));
    // flip i = the row locked by accepted column 90 - i (least reliable basis members first): that column's lane publishes the INDEX of its
    // pivot row (its column is the unit vector of that row); all 91 basis members exist, so every flip i < nflip <= 91 gets its entry
    int* fri = L.frow();
#define OSD_ROWIDX(X0, X1, X2) ((X0) ? __builtin_ctz(X0) : (X1) ? 32 + __builtin_ctz(X1) : 64 + __builtin_ctz((X2) | 0x80000000u))
    { const int i = 90 - kk0; if (in0 && i >= 0 && i < nflip) fri[i] = OSD_ROWIDX(b.x00, b.x01, b.x02); }
    { const int i = 90 - kk1; if (in1 && i >= 0 && i < nflip) fri[i] = OSD_ROWIDX(b.x10, b.x11, b.x12); }
    { const int i = 90 - kk2; if (in2 && i >= 0 && i < nflip) fri[i] = OSD_ROWIDX(b.x20, b.x21, b.x22); }
#undef OSD_ROWIDX
    // hm = rows whose accepted column has hard decision 1 (OR of those unit vectors): order-0 codeword bit of a column = parity(column & hm)
    if (lane < 3) L.hmw[lane] = 0u;
    __syncthreads();
    {
        const uint32_t h0 = ((in0 && b.hs0) ? b.x00 : 0u) | ((in1 && b.hs1) ? b.x10 : 0u) | ((in2 && b.hs2) ? b.x20 : 0u);
        const uint32_t h1 = ((in0 && b.hs0) ? b.x01 : 0u) | ((in1 && b.hs1) ? b.x11 : 0u) | ((in2 && b.hs2) ? b.x21 : 0u);
        const uint32_t h2 = ((in0 && b.hs0) ? b.x02 : 0u) | ((in1 && b.hs1) ? b.x12 : 0u) | ((in2 && b.hs2) ? b.x22 : 0u);
        if (h0) atomicOr(&L.hmw[0], h0);
        if (h1) atomicOr(&L.hmw[1], h1);
        if (h2) atomicOr(&L.hmw[2], h2);
    }
    __syncthreads();
    const uint32_t hm0 = L.hmw[0], hm1 = L.hmw[1], hm2 = L.hmw[2];
    OT(4);
    // per column: bit i = flip i has a 1 in this column (i < 62), bit 63 = the order-0 codeword bit
    // Flip i's row is one bit position of the 91-bit column: its index is read as a SCALAR (a broadcast LDS read), the word it lies in
    // is a uniform three-way branch, and a column's flip bit costs a v_bfe_u32 and a v_lshl_or_b32 -- 6 vector instructions per flip
    // for the three register sets (the generic "column AND unit vector != 0" form: ~30; this loop was 900 of the ~5800 vector
    // instructions of an attempt, and the kernel is bound by their number: profiles/r05_notes.md).
    uint32_t f0l = 0, f1l = 0, f2l = 0;
    uint32_t f0h = (uint32_t)((__popc(b.x00 & hm0) + __popc(b.x01 & hm1) + __popc(b.x02 & hm2)) & 1) << 31,
             f1h = (uint32_t)((__popc(b.x10 & hm0) + __popc(b.x11 & hm1) + __popc(b.x12 & hm2)) & 1) << 31,
             f2h = (uint32_t)((__popc(b.x20 & hm0) + __popc(b.x21 & hm1) + __popc(b.x22 & hm2)) & 1) << 31;
#define OSD_FBIT(XA, XB, XC, FA, FB, FC, SH) { FA |= __builtin_amdgcn_ubfe(XA, bp, 1u) << (SH); FB |= __builtin_amdgcn_ubfe(XB, bp, 1u) << (SH); \
                                               FC |= __builtin_amdgcn_ubfe(XC, bp, 1u) << (SH); }
#define OSD_FLIPS(LO, HI, FA, FB, FC, SUB)                                                                                         \
    for (int i = (LO); i < (HI); i++) {                                                                                            \
        const int r = __builtin_amdgcn_readfirstlane(fri[i]);                                                                      \
        const uint32_t bp = (uint32_t)r & 31u, sh = (uint32_t)(i - (SUB));                                                         \
        if (r < 32) OSD_FBIT(b.x00, b.x10, b.x20, FA, FB, FC, sh)                                                                  \
        else if (r < 64) OSD_FBIT(b.x01, b.x11, b.x21, FA, FB, FC, sh)                                                             \
        else OSD_FBIT(b.x02, b.x12, b.x22, FA, FB, FC, sh)                                                                         \
    }
    OSD_FLIPS(0, nflipA < 32 ? nflipA : 32, f0l, f1l, f2l, 0)
    OSD_FLIPS(32, nflipA, f0h, f1h, f2h, 32)
    // back to natural column order
    L.ftab[ord0] = ((uint64_t)f0h << 32) | f0l; L.ftab[ord1] = ((uint64_t)f1h << 32) | f1l; if (has2) L.ftab[ord2] = ((uint64_t)f2h << 32) | f2l;
    if (WIDE) {                                            // flips 62 .. nflip - 1 into the second word
        uint32_t* ftabB = L.ftabB();
        uint32_t g0 = 0, g1 = 0, g2 = 0;
        OSD_FLIPS(OSD_FLIPS_A, nflip, g0, g1, g2, OSD_FLIPS_A)
        ftabB[ord0] = g0; ftabB[ord1] = g1; if (has2) ftabB[ord2] = g2;
    }
#undef OSD_FLIPS
#undef OSD_FBIT
    __syncthreads();
}

// CRC syndrome (the CRC is linear: each of its 14 bits is a masked parity, d_SYNM) of the 91-bit word whose bit v is bit(v)
template <class Bit> FT8_DEV unsigned osd_syndrome_of(Bit bit) {
    uint32_t ra = 0, rb = 0, rc = 0;
#pragma unroll 8
    for (int v = 0; v < 32; v++) { ra |= bit(v) << v; rb |= bit(32 + v) << v; rc |= bit(64 + (v < 27 ? v : 0)) << v; }
    rc &= (1u << 27) - 1;
    unsigned sy = 0;
#pragma unroll
    for (int k = 0; k < 14; k++)
        sy |= (unsigned)((__popc(ra & d_SYNM[k][0]) + __popc(rb & d_SYNM[k][1]) + __popc(rc & d_SYNM[k][2])) & 1) << k;
    return sy;
}
// ---- CRC syndromes of the flip rows and the order-0 codeword -> fsyn[]: lane i < min(nflip, 62) takes flip i, lane 63 the order-0
// codeword (flips 62.. in a second round).  The lane gathers its word as a 91-bit column set: its bit of every table entry
template <bool WIDE>
FT8_DEV void osd_syndromes(OsdLds& L, int lane, int nflip) {
    const int nflipA = WIDE ? OSD_FLIPS_A : nflip;
    const int bitsel = (lane < nflipA) ? lane : 63;
    // the lane reads only the 32-bit half of each entry that holds its bit (two addresses per read: both broadcast), then a
    // v_bfe_u32 and a v_lshl_or_b32 per entry
    const uint32_t* fh = reinterpret_cast<const uint32_t*>(L.ftab) + (bitsel >= 32 ? 1 : 0);
    const unsigned sy = osd_syndrome_of([&](int v) { return __builtin_amdgcn_ubfe(fh[2 * v], (uint32_t)bitsel & 31u, 1u); });
    if (lane < nflipA) L.fsyn[lane] = (uint16_t)sy;
    if (lane == 63) L.fsyn[OSD_MAXFLIP + 1] = (uint16_t)sy;
    if (lane == 0) L.fsyn[OSD_MAXFLIP] = 0;
    if (WIDE) {                                            // lane l takes flip 62 + l: bit l of the second word of every column
        const uint32_t* ftabB = L.ftabB();
        const unsigned syB = osd_syndrome_of([&](int v) { return (ftabB[v] >> (lane & 31)) & 1u; });
        if (OSD_FLIPS_A + lane < nflip) L.fsyn[OSD_FLIPS_A + lane] = (uint16_t)syB;
    }
    __syncthreads();
}

// ---- the trials, in the table's order: a lane tests one trial (the XOR of its syndromes); the first accepted one is the result.
// EXT: the opt-in message types mt (ft8rx_set_msg_types, ft8_valid77_ext with osd = true: free text and telemetry are never accepted here).
// AP7: the first valid trial (as osd_012 returns it, max_hd = 0) is then gated: its distance to the hard decisions of the un-overridden
// LLRs must be <= the setting's ap_max_hd.
template <bool WIDE, bool EXT, bool AP7>
FT8_DEV Att osd_trials(OsdLds& L, int lane, const OsdInput& in, const OsdHard& hard, const OsdArgs& a) {
    const bool has2 = lane < 46;
    const uint32_t* ftabB = L.ftabB();
    const unsigned syn_c = L.fsyn[OSD_MAXFLIP + 1];
    const uint64_t M1 = (1ull << 27) - 1, M2 = (1ull << 46) - 1;
    Att res; memset(&res, 0, sizeof(res)); res.n_its = -1;
    const int slot = in.slot, ipass = AP7 ? 7 : (slot < 5) ? 5 : 6;
    for (int base = 0; base < a.ntr; base += 64) {
        const int t = base + lane;
        bool hit = false; int i = OSD_MAXFLIP, j = OSD_MAXFLIP, q = OSD_MAXFLIP;
        if (t < a.ntr) {
            const uint32_t e = a.trials[t];
            i = e & 0xFF; j = (e >> 8) & 0xFF; q = (e >> 16) & 0xFF;
            if (i == OSD_NONE) i = OSD_MAXFLIP;
            if (j == OSD_NONE) j = OSD_MAXFLIP;
            if (q == OSD_NONE) q = OSD_MAXFLIP;
            hit = (syn_c ^ L.fsyn[i] ^ L.fsyn[j] ^ L.fsyn[q]) == 0;
        }
        uint64_t hits = __ballot(hit);
        if (!hits) continue;                                  // no CRC-consistent word among these 64 trials (the usual case)
        // slow path, in trial order: rebuild the candidate codeword (natural column order) from the per-column flip words, apply the
        // distance gate, run the validity predicate, log the reference's unpack() call; the first accepted trial wins
        bool done = false;
        while (hits && !done) {
            const int hl = __builtin_ctzll(hits);
            hits &= hits - 1;
            const int hi_ = __shfl(i, hl), hj = __shfl(j, hl), hq = __shfl(q, hl);
            const uint64_t msk = (1ull << 63) | ((hi_ < OSD_FLIPS_A) ? (1ull << hi_) : 0ull) | ((hj < OSD_FLIPS_A) ? (1ull << hj) : 0ull) |
                                 ((hq < OSD_FLIPS_A) ? (1ull << hq) : 0ull);
            uint32_t mskB = 0;                                // flips 62..90 (the "no flip" index 91 sets nothing)
            if (WIDE) mskB = ((hi_ >= OSD_FLIPS_A && hi_ < OSD_MAXFLIP) ? (1u << (hi_ - OSD_FLIPS_A)) : 0u) |
                             ((hj >= OSD_FLIPS_A && hj < OSD_MAXFLIP) ? (1u << (hj - OSD_FLIPS_A)) : 0u) |
                             ((hq >= OSD_FLIPS_A && hq < OSD_MAXFLIP) ? (1u << (hq - OSD_FLIPS_A)) : 0u);
            const int l2 = 128 + (has2 ? lane : 0);
            const int pb0 = WIDE ? __popc(ftabB[lane] & mskB) : 0, pb1 = WIDE ? __popc(ftabB[64 + lane] & mskB) : 0, pb2 = WIDE ? __popc(ftabB[l2] & mskB) : 0;
            const uint64_t w0 = __ballot((__popcll(L.ftab[lane] & msk) + pb0) & 1), w1 = __ballot((__popcll(L.ftab[64 + lane] & msk) + pb1) & 1),
                           w2 = __ballot(has2 && ((__popcll(L.ftab[l2] & msk) + pb2) & 1));
            const int hd = __popcll(w0 ^ hard.w0) + __popcll(w1 ^ hard.w1) + __popcll((w2 ^ hard.w2) & M2);
            if (a.max_hd > 0 && hd > a.max_hd) continue;      // gate (extension): no unpack() call beyond max_hd
            uint64_t lo = 0, hi = 0;
            const int r = ft8_crc_check<EXT>(w0, w1 & M1, &lo, &hi, a.mt, true);
            const int t = base + hl;
            if (r && lane == 0) log_event(a.ev, a.evcount, (int)(in.vec / 10) >> a.sh, (int)(in.vec / 10) & ((1 << a.sh) - 1), ipass, AP7 ? 2 * slot + 1 : slot, t, lo, hi, r == 2);   // a call the reference made (mode 0: vec = candidate * 10 + slot)
            if (r == 2) {
                res.ok = 1; res.lo = lo; res.hi = hi; res.n_its = (int16_t)t;
                if constexpr (AP7) res.ok = hd <= a.apc->max_hd;
                res.method = (AP7 || slot < 5) ? FT8RX_M_OSD : FT8RX_M_LDPC_B_OSD;
                res.pad[0] = (uint8_t)hd;                     // Hamming distance of the accepted codeword to the hard decisions
                done = true;
            }
        }
        if (done) break;
    }
    return res;
}

// One attempt = one wavefront: the phases in order, the timing marks of tools/osd_timing.py between them.  The result goes to
// attO[vec] (mode 0: candidate * 10 + slot; AP7: candidate * 10 + pattern - 5; mode 2: the vector's index).
// WIDE: more than 62 flip rows (k_osd*_wide) -- kernels of their own, because the second flip word costs 13 VGPRs = two of the waves per
// SIMD that hide this kernel's scalar-pipe latency (one kernel with a run-time switch: 0.737 -> 0.791 ms per 256 frames at the
// reference's 30 / 2)
template <bool WIDE, bool NANV, bool EXT = false, bool AP7 = false>
FT8_DEV void osd_attempt(int lane, int mode, int bid, const OsdArgs& a) {
    __shared__ OsdLds L;
    OsdClock ot;
    const OsdInput in = osd_load<AP7>(L, lane, mode, bid, a);
    if (!in.go) return;
    uint32_t ix[3];
    if (!osd_order<NANV>(L, lane, bid, a.nanlist, ix, ot)) return;
    OT(1);
    const OsdHard hard = osd_hard(in.hsrc, lane);
    const OsdBasis basis = osd_eliminate(L, lane, ix, ot);
    OT(3);
    osd_flip_table<WIDE>(L, lane, ix, basis, a.nflip, ot);
    OT(5);
    osd_syndromes<WIDE>(L, lane, a.nflip);
    OT(6);
    const Att res = osd_trials<WIDE, EXT, AP7>(L, lane, in, hard, a);
    OT(7);
    if (lane == 0) a.attO[in.vec] = res;
    OT_FLUSH;
}

// Eight waves per SIMD: the elimination is a serial chain of readlane -> scalar logic -> masked XOR per step (~280 cycles), hidden only
// by other waves.  The kernel needs 52 VGPRs when told to fit eight (it took 71 when it was not) and 4.5 KB of LDS since the flip rows
// share the work area of the elimination (5.6 KB allowed 7): 0.739 -> 0.710 ms per 256 frames (profiles/archive/r03_notes.md; the attribute alone, LDS-bound at 7: 0.781)
#ifndef OSD_ATTR
#define OSD_ATTR __attribute__((amdgpu_waves_per_eu(8, 8)))
#endif
// The family's driver: blocks stride over n attempts, id(item) = the attempt's bid.  One body of osd_attempt per kernel: k_osd*_wide fit
// their 64 VGPRs with no more scratch than they had only while nothing else of the kernel keeps a register across the attempt.
template <bool WIDE, bool NANV, bool EXT, bool AP7, class Id>
FT8_DEV void osd_blocks(int n, int mode, const OsdArgs& a, Id id) {
#pragma unroll 1
    for (int item = blockIdx.x; item < n; item += gridDim.x) {
        int lane = threadIdx.x;
        asm volatile("" : "+v"(lane));       // opaque per item: nothing lane-specific is hoisted across attempts (register pressure)
        osd_attempt<WIDE, NANV, EXT, AP7>(lane, mode, id(item), a);
        __syncthreads();                     // the LDS struct is reused by the next attempt
    }
}
// mode 2 (test entry): one block per vector.  Pipeline: blocks stride over OSD work list x 10 attempts (5 AP variants of the fine LLRs, then the 5
// saved BP outputs).  NaN kernels: over the attempts the main ones left on `nanlist` (ids as they got them: candidate * 10 + slot, or the vector's index).
// k_osd* : a handle with msg_types = 0 (the reference's predicate); k_osd*_ext: msg_types != 0, passed as the last argument
#define OSD_PARAMS int mode, const float* __restrict__ llr_in, const float* __restrict__ saved, const Att* __restrict__ attB,       \
                   ft8rx_record* __restrict__ rec, const int32_t* __restrict__ ncand, Att* __restrict__ attO, ft8rx_event* ev,      \
                   int32_t* evcount, const uint32_t* __restrict__ trials, int ntr, int nflip, int max_hd, int sh
#define OSD_KERNEL(NAME, NAN_NAME, WIDE, EXT, MT_PARAM, MT)                                                                          \
__global__ __launch_bounds__(64) OSD_ATTR void NAME(OSD_PARAMS, WorkList work, WorkList nanlist MT_PARAM) {                         \
    const OsdArgs a = {llr_in, saved, attB, rec, ncand, attO, ev, evcount, trials, ntr, nflip, max_hd, sh, nanlist, MT, nullptr};   \
    osd_blocks<WIDE, false, EXT, false>(mode == 2 ? (int)gridDim.x : *work.count * 10, mode, a,                                     \
                                        [&](int item) { return mode == 2 ? item : work.items[item / 10] * 10 + item % 10; });       \
}                                                                                                                                   \
__global__ __launch_bounds__(64) void NAN_NAME(OSD_PARAMS, WorkList nanlist MT_PARAM) {                                             \
    const OsdArgs a = {llr_in, saved, attB, rec, ncand, attO, ev, evcount, trials, ntr, nflip, max_hd, sh, nanlist, MT, nullptr};   \
    osd_blocks<WIDE, true, EXT, false>(*nanlist.count, mode, a, [&](int item) { return nanlist.items[item]; });                     \
}
#define OSD_MT_PARAM , unsigned mt
OSD_KERNEL(k_osd, k_osd_nan, false, false, , 0u)
OSD_KERNEL(k_osd_wide, k_osd_nan_wide, true, false, , 0u)        /* more than OSD_FLIPS_A flip rows */
OSD_KERNEL(k_osd_ext, k_osd_nan_ext, false, true, OSD_MT_PARAM, mt)
OSD_KERNEL(k_osd_wide_ext, k_osd_nan_wide_ext, true, true, OSD_MT_PARAM, mt)
#undef OSD_KERNEL
#undef OSD_PARAMS
#undef OSD_MT_PARAM
#define OSD_NAN_GRID 512             /* blocks of the NaN kernels: they stride over a list that is almost always empty */

#endif
