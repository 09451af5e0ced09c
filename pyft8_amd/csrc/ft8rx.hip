// ft8rx.hip -- MI355X (gfx950) FT8 receive hot path: HIP kernels + the C ABI of include/ft8rx.h.
//
// Pipeline for a batch of B independent 15-s frames (stream-ordered, no host
// round trips; frames are the batch dimension, candidates the second one):
//   k_spectrogram  (hop, frame)         Hann * 3840-pt real FFT (1920-pt complex Stockham in LDS) -> dB grid
//   k_sync         (16-f0 tile, frame)  Costas correlation over all time offsets from an LDS tile
//   k_topk         (frame)              threshold + stable top-K (bitonic sort in LDS)
//   k_grid_llr     (candidate)          payload gather -> max-log LLRs -> sigma normalisation
//   k_bp           (candidate, AP)      one wavefront: GOOD91 + flooding BP, ballot parity, LDS exchange
//   k_select0      (candidate)          first success in ladder order
//   k_cyc_a/bc     (tile, frame)        192000-pt real FFT as 300x320 four-step; row pass fused with the real split
//   k_fine         (candidate)          9x(slice/taper/3200-pt IFFT) + 32-pt DFT scoring, Costas gate, LLRs
//   k_bp           (candidate, AP)      GOOD91 + BP(90,20) with saved outputs
//   k_select1, k_osd (candidate, slot) one wavefront: rank sort, register-resident GF(2) Gauss-Jordan
//                                       with ballot pivoting, lane-per-trial CRC-14 + validity, k_select2
//   k_bp_ap, k_osd_ap (cand, pattern)   opt-in ipass 7 (ft8rx_set_ap_calls): the operator's and the DX station's calls as known bits,
//                                       only while a call is set (kernels/ap_calls.hpp)
//   k_sync3, k_fine_weak                opt-in weak mode (ft8rx_set_weak): the sync search and the fine sync scored on all three Costas
//                                       blocks, a wide joint fine scan, no sd gates, an OSD distance gate
//   k_fine (trip), k_recall_score       opt-in ipass 8 (ft8rx_set_recall): forced fine sync at the positions of messages heard 30 s
//                                       earlier and a hypothesis test per entry, only for a batch with entries (kernels/recall.hpp)
//   k_report_worklist, k_report         opt-in measured reports (ft8rx_set_reports): SNR, frequency and start time of every DECODED
//                                       record from a matched correlation with its own 79 tones (kernels/report.hpp)
// A batch is cut into chunks whose chains run on separate HIP streams -- free-running: chunk i of batch k+1 follows chunk i of batch k
// on stream i, no per-batch fork / join; results land in one of two result slots and are copied to page-locked host buffers by a copy
// stream while the next batch computes; the used part of the event log is packed by k_ev_scan / k_ev_compact straight into
// page-locked host memory (batch_plan.hpp; launch_batch = batch_begin, batch_submit, batch_finish; ft8rx_fetch_results).
// k_sub_* / k_subd_* subtract decoded signals (ft8rx_subtract; refine 0 = the reference experiment's subtract_signal,
// 3 = its refine_time_origin first: k_cyc_a_f32 + k_refine3; 1 / 2 = the build's own origin re-estimation).
// Reference line citations are to PyFT8/receiver.py and PyFT8/decoders.py (see include/ft8rx.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include "../../include/ft8rx.h"
#include "ft8_dev.h"
#include "sample_fmt.hpp"

#define WL_MULT(i) ((i) == WL_BP0 ? 5 : (i) == WL_OSDNAN ? 10 : 1)      /* entries per candidate slot of work list i */
#define NF0MAX (FT8RX_MAX_F0 > 1024 ? 2048 : 1024)     /* per-frame stride of the per-f0 sync results; k_topk sorts this many keys */

// The kernels live in one file per stage; this file is the C ABI, the handle and the launch chains.
#include "kernels/common.hpp"
#include "kernels/spectrogram.hpp"
#include "kernels/sync_search.hpp"
#include "kernels/llr.hpp"
#include "kernels/ap_patterns.hpp"
#include "kernels/bp.hpp"
#include "kernels/cycle_spectrum.hpp"
#include "kernels/fine_sync.hpp"
#include "kernels/osd.hpp"
#include "kernels/ap_calls.hpp"
#include "kernels/recall.hpp"
#include "kernels/report.hpp"
#include "kernels/sample.hpp"
#include "kernels/ddc.hpp"
#include "kernels/ddc_wide.hpp"
#include "kernels/ddc_rat.hpp"
#include "kernels/blanker.hpp"
#include "kernels/blank_in.hpp"
#include "kernels/pan.hpp"
#include "kernels/ft4.hpp"
#include "kernels/ft4_weak.hpp"     // after ft4.hpp: it shares the sample read, the Costas tables and the range
#include "kernels/ft4_verify.hpp"   // after ft4.hpp and recall.hpp: it shares the sample read, the Costas tables and the device encoder
#include "kernels/synth.hpp"
#include "kernels/subtract.hpp"
#include "kernels/ft4_sub.hpp"      // after subtract.hpp: it shares wave_sum2 and the int16 <-> float32 copies
#include "kernels/ft4_report.hpp"   // after ft4_sub.hpp: it walks the subtraction's model
#include "kernels/probes.hpp"
#include "host_messages.hpp"
#include "batch_plan.hpp"
#include "ddc_ring.hpp"
#include "ddc_frames.hpp"
#include "ddc_grid_ring.hpp"
#include "ddc_wide_ring.hpp"
#include "ddc_rat_ring.hpp"
#include "blank_in_ring.hpp"
#include "pan_ring.hpp"
#include "optins.hpp"
#include "ilp_launch.hpp"       // k_fine, k_spectrogram and k_hop_spectrum are launched from the second translation unit (ft8rx_ilp.hip)

// ====================================================================================== host side
#define EV_EAGER_BYTES ((size_t)1 << 20)      /* event logs up to this size travel whole with the records (batch_finish) */
#define HIPCHK(h, x) do { hipError_t _e = (x); if (_e != hipSuccess) { set_err(h, "%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); return -2; } } while (0)

// OSD trial list in the reference's order (decoders.py:248-272): order 0; single flips i < S; the restricted double flips
// (i, j), i < S, j < min(i, D), i-major; then the build's order-3 extension (i, j, k), k < j < i < T, i-major.  One packed entry
// per trial: i | j << 8 | k << 16, OSD_NONE for "no flip".
static std::vector<uint32_t> osd_trial_table(int S, int D, int T) {
    std::vector<uint32_t> t;
    const uint32_t N = OSD_NONE;
    t.push_back(N | (N << 8) | (N << 16));
    for (int i = 0; i < S; i++) t.push_back((uint32_t)i | (N << 8) | (N << 16));
    for (int i = 0; i < S; i++) for (int j = 0; j < D && j < i; j++) t.push_back((uint32_t)i | ((uint32_t)j << 8) | (N << 16));
    for (int i = 0; i < T; i++) for (int j = 0; j < i; j++) for (int k = 0; k < j; k++) t.push_back((uint32_t)i | ((uint32_t)j << 8) | ((uint32_t)k << 16));
    return t;
}
static int osd_nflip(int S, int T) { return S > T ? S : T; }

struct ft8rx_hashes { hostmsg::Hashes H; };      // persistent call-hash table (databases.py:8): ft8rx_hashes_* in include/ft8rx.h

// k_sync holds every grid row its h0 window can touch in LDS (244 B per row): windows of at most SYNC_WIN time offsets per launch.  A
// wider search_time_range runs as consecutive windows in ascending h0, each launch keeping the earlier windows' maximum unless it
// finds a strictly larger one -- the first strict maximum of the whole range (receiver.py:350-351), as one launch gives it.
#define SYNC_WIN 352
static size_t sync_lds_bytes(const ft8rx_config& c) {
    const int nh0 = c.h0_hi - c.h0_lo;
    const size_t nrows = (size_t)((nh0 < SYNC_WIN ? nh0 : SYNC_WIN) + 24);
    return nrows * 16 * sizeof(double) + (nrows * 29 + 512) * sizeof(float);
}
static std::string g_create_err;

// Result slots.  A batch writes its records / events into slot k % 2 and, when its kernels are done, the copy stream moves them into
// page-locked host buffers while the next batch computes into the other slot; ft8rx_fetch_results hands out the oldest unfetched
// batch.  At most two batches' results are retained.  Everything a batch leaves behind lives here, once per slot.
struct ResultSlot {
    ft8rx_record* rec = nullptr; int32_t* ncand = nullptr; ft8rx_event* ev = nullptr; int32_t* evcount = nullptr;      // on the device
    ft8rx_record* h_rec = nullptr; int32_t* h_cnt = nullptr; ft8rx_event* h_ev = nullptr; int32_t* h_evc = nullptr;    // page-locked copies
    hipEvent_t ev_comp = nullptr, ev_done = nullptr;     // the batch's kernels are done / its results have reached the host buffers
    int B = 0;                                           // frames of the batch the slot holds
    // Large batches (event log > EV_EAGER_BYTES): k_ev_scan / k_ev_compact pack the used entries of the log and write them straight
    // into page-locked host memory (h_evpacked; d_evpacked = the same buffer's device address); the fetch spreads them over h_ev's
    // [frame][cap] rows (fetch_events)
    bool evpending = false;
    int32_t* d_evoffs = nullptr; ft8rx_event* h_evpacked = nullptr; ft8rx_event* d_evpacked = nullptr;
    // packed results (ft8rx_set_packed_output): the caller's buffer (as a device address), a page-locked mirror of its header, and
    // ft8rx_packed_output_fence's event: the consumer's "done reading this buffer"
    bool packed = false;
    unsigned char* pk_buf = nullptr; hipEvent_t pk_fence = nullptr;
    ft8rx_packed_header* h_pkhdr = nullptr; ft8rx_packed_header* d_pkhdr = nullptr;
    // recall (ft8rx_set_recall): the batch's entry copy and results
    bool recall = false;
    ft8rx_recall_entry* d_rc_ent = nullptr; int32_t* d_rc_cnt = nullptr; ft8rx_record* d_rc_rec = nullptr;
    ft8rx_record* h_rc_rec = nullptr; int32_t* h_rc_cnt = nullptr;
    // measured reports (ft8rx_set_reports): [max_frames][stride] on the device
    bool reports = false;
    ft8rx_report* d_rp = nullptr; ft8rx_report* h_rp = nullptr;
};

static ApCalls ap_calls_off() { ApCalls a; memset(&a, 0, sizeof(a)); a.max_hd = FT8RX_AP_MAX_HD_DEFAULT; return a; }

#ifndef LADDER_GRID_CAP
#define LADDER_GRID_CAP (4 * 256 * 32)
#endif

// The front stage of a rate, filled from the plan by pre_plan: ONE stream at `rate` -> per channel IQ float32 at
// rate_mid = rate L / M through a per-channel table of the n_taps prototype taps.  The wide pre-decimator is L = 1, M = R0.
enum { PRE_WIDE = 0, PRE_RAT = 1 };
static const char* const PRE_NAME[2] = {"wide", "rational"};                       // in messages
static const char* const PRE_ENTRY[2] = {"ft8rx_ddc_wide", "ft8rx_ddc_rat"};
static const uint32_t PRE_KINDS[2] = {SF_KINDS_WIDE, SF_KINDS_RAT};                 // the kinds each takes (sample_fmt.hpp)
struct PreStage {
    int which = PRE_WIDE;
    int32_t rate = 0, rate_mid = 0;              // rate_mid = 0: the rate is refused
    int L = 1, M = 1, n_taps = 0;
    int P = 0, H = 0, tk = 0; bool lane = false; // taps per phase (rational), history of a stream, outputs per tile, the rational kernel's regime
    const std::vector<float>* taps = nullptr;    // the prototype (pre_taps); nullptr: the rate is refused
    int64_t n_max = 0, end_max = 0;              // bound of an origin, and of the index a stream may reach
    const char *name = "", *entry = "";          // PRE_NAME, PRE_ENTRY of `which`
};

struct ft8rx_handle {
    ft8rx_config cfg = {};
    int device = 0, max_frames = 0;
    hipStream_t stream = nullptr;
    int n_streams = 2;                   // chunks of a batch run their kernel chains on separate streams
    int ladder_mode = 0;                 // fine-stage BP launches: 0 = ladder order (three launches), 1 = one launch (ft8rx_set_ladder_mode)
    int ladder_cap = LADDER_GRID_CAP;    // most blocks a ladder kernel is launched with (ladder_grid; ft8rx_set_ladder_grid)
    int msg_types = 0;                   // opt-in message types, FT8RX_MT_* bits (ft8rx_set_msg_types; 0 = the reference's rule)
    // opt-in weak mode (ft8rx_set_weak; off = the reference's stages)
    bool weak = false; float weak_sync_min = FT8RX_WEAK_SYNC_MIN_DEFAULT; int32_t weak_osd_max_hd = FT8RX_WEAK_OSD_MAX_HD_DEFAULT;
    ApCalls ap = ap_calls_off();         // ipass-7 patterns (ft8rx_set_ap_calls; ap.np = 0: off), as the host last set them
    // the setting's version, and the version each chunk's device copy holds
    uint32_t ap_version = 0, ap_chunk_version[batchplan::MAX_CHUNKS] = {};
    ApCalls* d_apc = nullptr;            // [MAX_CHUNKS] per-chunk device copies of `ap`, written on the chunk's stream (enqueue_chain)
    int32_t* d_apcount = nullptr;        // [MAX_CHUNKS][2] ipass-7 list lengths per chunk: candidates, OSD attempts
    // recall (ft8rx_set_recall, kernels/recall.hpp; allocated on first use): the pending entries of the next batch and its per-frame
    // triple offsets (host copy rc_off) and the forced fine sync's scratch; the batch's entry copy and results are its ResultSlot's
    bool rc_armed = false; int rc_frames = 0; bool rc_td = false; std::vector<int32_t> rc_off;
    int32_t rc_max_hd = FT8RX_RECALL_MAX_HD_DEFAULT, rc_min_gap = FT8RX_RECALL_MIN_GAP_DEFAULT;
    ft8rx_recall_entry* d_rc_src = nullptr; int32_t* d_rc_srccnt = nullptr; int32_t* d_rc_off = nullptr;
    int32_t* d_rc_trip = nullptr; int32_t* d_rc_tout = nullptr; float* d_rc_tsd = nullptr; float* d_rc_sgrid = nullptr; float* d_rc_llr = nullptr;
    // measured reports (ft8rx_set_reports, kernels/report.hpp; allocated at the first ft8rx_set_reports(h, 1)): the work list of the
    // DECODED slots ([max_frames][stride] ids, a counter per chunk); the reports themselves are the ResultSlot's
    bool reports = false;
    int32_t* d_rp_items = nullptr; int32_t* d_rp_count = nullptr;
    int sub_frames = FT8RX_SUBBATCH_DEFAULT;     // frames per kernel chain inside a chunk (ft8rx_set_subbatch; 0 = the whole chunk in one chain)
    hipStream_t sub[batchplan::MAX_STREAMS] = {};
    hipEvent_t ev_fork = nullptr, ev_join[batchplan::MAX_STREAMS] = {};
    hipStream_t copy_s = nullptr;    // host-to-device chunk copies of ft8rx_decode_batch, in order, never queued behind kernels
    hipEvent_t ev_chunk[batchplan::MAX_CHUNKS] = {};
    Tables T = {};
    std::vector<void*> allocs, pinned;   // everything the handle owns: device memory (dalloc) and page-locked host memory (halloc)
    unsigned ready = 0;                  // the lazily created workspace groups that are complete, 1 << WS_* (FirstUse)
    struct Chunk { void* p; size_t cap, used; };
    std::vector<Chunk> arena;        // scratch of the stage entry points (struct Scratch)
    int16_t* d_audio = nullptr;  // staging for host-pointer entry points
    int16_t* d_audio2 = nullptr; // second staging buffer (allocated on first use): ft8rx_enqueue_batch_host double-buffers the H2D copies
    float* d_audio_f = nullptr;  // float32 frames (allocated on first use): the staging of the _f32 host entries ...
    float* d_audio2_f = nullptr; // ... and the second buffer of ft8rx_enqueue_batch_host_f32
    hipStream_t h2d_s = nullptr; // host-to-device copies of the pipelined host entry: never queued behind kernels or result copies
    float* d_grid = nullptr;
    float* d_best_score = nullptr; int32_t* d_best_h0 = nullptr;
    // slot 0's device buffers under the names the stage entry points use
    ft8rx_record* d_rec = nullptr; int32_t* d_ncand = nullptr; ft8rx_event* d_ev = nullptr; int32_t* d_evcount = nullptr;
    float* d_llr0 = nullptr; float* d_saved = nullptr;
    Att *d_att0 = nullptr, *d_attG = nullptr, *d_attB = nullptr, *d_attO = nullptr;
    cpx *d_A = nullptr, *d_spec = nullptr;
    const uint32_t* d_trials = nullptr; int n_trials = 0;      // OSD trial list of this configuration
    int32_t* d_work[WL_N] = {};                  // ladder work lists (kernels/common.hpp: WorkList), [B][stride] candidate ids each
    int32_t* d_wcount = nullptr;                 // [MAX_CHUNKS][WL_N] list lengths, zeroed at the head of every chunk's chain
    uint8_t* d_colmask = nullptr; bool use_mask = false;      // [B][NF0MAX] search mask of the local re-search (ft8rx_set_search_mask), allocated on first use
    ResultSlot slots[2];
    // the slot the next batch writes, the oldest unfetched one, how many are unfetched, the latest batch's, the one fetched last
    int slot_enq = 0, slot_fetch = 0, inflight = 0, last_slot = -1, fetched_slot = -1;
    // free-running chunk streams (batch_submit): the chunk chains of consecutive batches follow each other on their own streams
    // without a per-batch fork / join; need_barrier = something else has used the shared workspaces (or the partition changed) since
    hipEvent_t ev_cdone[2][batchplan::MAX_STREAMS] = {};
    bool free_running = false, need_barrier = true; int part_B = 0, part_n = 0;
    // packed results (ft8rx_set_packed_output): the capacity of each slot's buffer and the scratch of the pack kernels
    uint64_t pk_cap = 0; uint64_t* d_pkneed = nullptr; int32_t* d_pknrec = nullptr;
    hipEvent_t d2h_ev[32] = {}; uint32_t d2h_next = 0;      // ft8rx_d2h_async: tickets (a ring of events on the result-copy stream)
    // signal subtraction (extension, allocated on first use): float32 working copy, per-chunk partial sums, GFSK tables
    float* d_wf = nullptr; double2* d_part = nullptr; double* d_pulse = nullptr; double* d_pc = nullptr;
    ft8rx_subsig* d_sigs = nullptr; int32_t* d_sigcnt = nullptr; int sig_cap = 0;
    float2 *d_zdec = nullptr, *d_model = nullptr, *d_adec = nullptr; SubdCtx* d_subctx = nullptr;      // decimated-baseband refinement (refine = 2), allocated on first use
    double* d_ones = nullptr;                                   // refine = 3: an all-ones taper table
    // down-converter (ft8rx_ddc, kernels/ddc.hpp; allocated on first use): the channel table of a call, [max_frames]; the input
    // staging of ft8rx_ddc_host, grown when a call needs more
    // (h_ddc_outs: its page-locked source; ddc_ev: behind the copy of the last call's table, so that the next call can rewrite it)
    DdcOut* d_ddc_outs = nullptr; DdcOut* h_ddc_outs = nullptr; hipEvent_t ddc_ev = nullptr; void* d_ddc_in = nullptr; size_t ddc_in_cap = 0;
    // streaming down-converter (ft8rx_ddc_stream_*): everything is allocated by open and released by close (or
    // destroy); it shares nothing but the tap tables with the one-shot above.  d_in: [n_streams][cap] samples of `fmt`, the newest cap
    // of each stream; d_out / d_f32: [n_out][OUT_RING]; h_stage: page-locked, one second of every stream; ev: behind the last copy out
    // of h_stage.  n_origin, pushed, tiles: absolute index of the first sample, samples pushed, first tile not produced yet.
    // The spectrogram stage behind it (ft8rx_ddc_stream_grid_*, section 16.5; nothing of it exists until grid_open): d_grid
    // [n_out][g_rows][FT8RX_GRID_COLS], row q at q mod g_rows; g_p0: the hop phase.
    struct DdcStream {
        bool open = false; int fmt = 0, D = 0, n_streams = 0, n_out = 0; int32_t rate = 0; float scale = 0.0f;
        int64_t n_origin = 0, pushed = 0, tiles = 0, cap = 0;
        void* d_in = nullptr; int16_t* d_out = nullptr; float* d_f32 = nullptr; DdcOut* d_outs = nullptr; char* h_stage = nullptr;
        float* d_grid = nullptr; int g_p0 = 0, g_rows = 0;
        bool f32_frames = false;         // opened with keep_f32 = FT8RX_DDC_KEEP_F32_FRAMES: the grid stage reads d_f32
        // ft8rx_ddc_stream_frames (section 19.7; nothing of it exists until the stream's first such call): d_sel [max_frames], the
        // channel of each frame of the last call's list, and that list on the host -- uploaded only when a call's list differs
        int32_t* d_sel = nullptr; std::vector<int32_t> sel;
        hipEvent_t ev = nullptr;
    } ds;
    // input pre-stages (ft8rx_ddc_wide*, ft8rx_ddc_rat*; kernels/ddc_wide.hpp, kernels/ddc_rat.hpp).  One-shot: the
    // channels' tap tables and frequency words, and the intermediate samples [n_out][n_mid], each grown when a call needs more (one
    // call at a time uses them, whichever stage it runs).
    void* d_pre_tab = nullptr; size_t pre_tab_cap = 0; void* d_pre_w0 = nullptr; size_t pre_w0_cap = 0;
    void* d_pre_mid = nullptr; size_t pre_mid_cap = 0;
    // ... and their stream, at most one of either stage: everything is allocated by open and released by close (or destroy).  st: the
    // stage of the open stream; d_hist: the newest st.H input samples in their own format `fmt` (sample n at (n - n_origin) mod H); d_chunk /
    // h_stage: one second of input, device / page-locked; d_mid: [n_out][rate_mid], what one push makes; the down-converter behind it
    // is the stream `ds` above, fed on the device.  n_origin, pushed, k_done: absolute index of the first sample, samples pushed, first
    // intermediate sample not made yet.
    struct PreStream {
        bool open = false; PreStage st; int fmt = 0, n_out = 0;
        int64_t n_origin = 0, pushed = 0, k_done = 0;
        char* d_hist = nullptr; char* d_chunk = nullptr; char* h_stage = nullptr; float2* d_mid = nullptr; float2* d_tab = nullptr;
        uint32_t* d_w0 = nullptr;
        hipEvent_t ev = nullptr;
    } ps;
    // noise blanker (ft8rx_blank, kernels/blanker.hpp; allocated on first use): (m_b, L_b) [max_frames][375][2], the
    // hit mask [max_frames][2813] 64-bit words, the counters' tile partials [max_frames][88][4], the counters [max_frames][4] and the
    // taper tables [65][65]
    int32_t* d_bl_lv = nullptr; uint64_t* d_bl_mask = nullptr; int32_t* d_bl_part = nullptr; int32_t* d_bl_stats = nullptr; int32_t* d_bl_taper = nullptr;
    // input-rate noise blanker (ft8rx_blank_in*, kernels/blank_in.hpp).  BlankInWs: what one run works in -- the
    // level ring [lv_cap][2], the hit mask ring (mask_words 64-bit words), the partial counters of one hit and one gate launch
    // [part_cap][2] each, the cumulative counters int64[4].  bi: the one-shot entries' (first use, grown on demand), with the host
    // entry's sample buffer d_bi_buf; d_bi_taper: the taper tables [65][65].  bis: the stream -- everything allocated by open and
    // released by close (or destroy): two work buffers used in turn ([leftover | chunk], `base` = absolute index of the current one's
    // first sample), the page-locked chunk.
    struct BlankInWs {
        int32_t* d_lv = nullptr; size_t lv_cap = 0; uint64_t* d_mask = nullptr; size_t mask_words = 0;
        int32_t* d_part_h = nullptr; int32_t* d_part_g = nullptr; size_t part_cap = 0; long long* d_stats = nullptr;
    } bi;
    char* d_bi_buf = nullptr; size_t bi_buf_cap = 0; int32_t* d_bi_taper = nullptr;
    struct BlankInStream {
        bool open = false, finished = false; int fmt = 0, log2_b = 0, guard = 0, taper = 0, cur = 0; int32_t threshold_q8 = 0;
        int64_t n_origin = 0, pushed = 0, max_push = 0, base = 0;
        char* d_work[2] = {nullptr, nullptr}; char* h_stage = nullptr;
        BlankInWs ws;
        hipEvent_t ev = nullptr;
    } bis;
    // panorama (ft8rx_pan*, kernels/pan.hpp).  PanWs: what a run works in -- the window's weights [n_fft], the
    // powers [tile_w][bins] and statistics [tile_w][2] of one tile of windows, the rows [slots][bins] and their statistics [slots][2].
    // d_pan_tw: the twiddles [8192], made with the one-shot entries' weight table at the first use of either.  pan: the one-shot
    // entries' (grown on demand; slots = the rows of the call), with the host entry's sample buffer d_pan_in.  pans: the stream --
    // everything allocated by open and released by close (or destroy): the work buffer [leftover | chunk], the leftover's own copy,
    // the page-locked chunk.
    struct PanWs { float* d_win = nullptr; int win_n = 0; float* d_pw = nullptr; int32_t* d_wstat = nullptr; size_t tile_w = 0;
                   float* d_ring = nullptr; int32_t* d_rstat = nullptr; size_t slots = 0; } pan;
    cpx* d_pan_tw = nullptr; size_t pan_pw_cap = 0, pan_wstat_cap = 0, pan_ring_cap = 0, pan_rstat_cap = 0;
    void* d_pan_in = nullptr; size_t pan_in_cap = 0;
    struct PanStream {
        bool open = false; int fmt = 0, N = 0, A = 0, n_rows = 0;
        int64_t n_origin = 0, pushed = 0, max_push = 0;
        char* d_work = nullptr; char* d_left = nullptr; char* h_stage = nullptr;
        PanWs ws;
        hipEvent_t ev = nullptr;
    } pans;
    // FT4 (ft8rx_ft4_*, kernels/ft4.hpp; everything allocated at the first FT4 call, WS_FT4): the knobs and the search
    // range; frames [max_frames][90000], the dB grid [max_frames][618][577], the FFT's tables, the per-f0 maxima before / after
    // k_ft4_peaks [max_frames][NF0MAX]; per candidate slot ([max_frames << cand_shift]) the triples, LLRs, BP outputs, tweaks, metric,
    // SNR, BP and OSD attempts, the OSD list, its dense LLR rows and its NaN list; the two list counters and their page-locked copy
    struct Ft4 {
        float sync_min = FT8RX_FT4_SYNC_MIN_DEFAULT; int32_t osd_max_hd = FT8RX_FT4_OSD_MAX_HD_DEFAULT;
        Ft4Range range = {2, 567, -42, 168};     // 12.5 .. 5900 Hz, -0.5 .. +2.0 s
        size_t bytes = 0;
        int16_t* d_audio = nullptr; float* d_grid = nullptr; float* d_win = nullptr; cpx* d_w576 = nullptr; cpx* d_wr = nullptr;
        float* d_raw = nullptr; float* d_kept = nullptr; int32_t* d_bh = nullptr;
        int32_t* d_trip = nullptr; float* d_llr = nullptr; float* d_saved = nullptr; int32_t* d_tweak = nullptr; float* d_metric = nullptr;
        int32_t* d_snr = nullptr; Att* d_att = nullptr; Att* d_attO = nullptr; int32_t* d_items = nullptr; float* d_dense = nullptr;
        int32_t* d_nan = nullptr; int32_t* d_count = nullptr; int32_t* h_count = nullptr;
    } ft4;
    // FT4 subtraction (ft8rx_ft4_subtract / _sub_probe, kernels/ft4_sub.hpp; allocated at the first of those calls, WS_FT4_SUB): the
    // float32 working copy [max_frames][90000], the partial bins [max_frames][13][6][41], the pulse's running sum [1729], and per row
    // the winning trial, the signal count, the frame of a probe row, the 13 energies and FT4SUB_MAXSIGS signals
    struct Ft4Sub {
        size_t bytes = 0;
        float* d_wf = nullptr; double2* d_part = nullptr; double* d_pc = nullptr; int32_t* d_best = nullptr; int32_t* d_cnt = nullptr;
        int32_t* d_frame = nullptr; double* d_energy = nullptr; ft8rx_ft4_subsig* d_sigs = nullptr;
    } ft4sub;
    // FT4 measured reports (ft8rx_ft4_report, kernels/ft4_report.hpp; allocated at the first call,
    // WS_FT4_REPORT): the float32 frames [max_frames][90000] (zero from n_have on), a pulse table of its own, and per row of a slab
    // (one signal per row, FT4REP_ROWS x max_frames rows): the signal, its frame, a count of 1, the partial scores [26][169], the
    // scores [169], the peak, the report and (on, off)
    struct Ft4Rep {
        size_t bytes = 0;
        float* d_wf = nullptr; double* d_pc = nullptr; ft8rx_ft4_subsig* d_sigs = nullptr; int32_t* d_frame = nullptr; int32_t* d_one = nullptr;
        float* d_part = nullptr; float* d_scores = nullptr; Ft4RepPeak* d_peak = nullptr; ft8rx_report* d_rep = nullptr; float* d_onoff = nullptr;
    } ft4rep;
    // FT4 coherent LLRs (ft8rx_ft4_set_coherent, k_ft4_coh; allocated at the first FT4 batch that runs with the
    // setting on, WS_FT4_COH).  Per item of the failure list (at most max_frames << cand_shift): q, the nine metrics, the run-of-2 rows
    // and behind them the run-of-4 rows, BP's outputs and attempts for both, the list OSD gets, its counter and the page-locked copy
    struct Ft4Coh {
        bool on = false; size_t bytes = 0;
        int32_t* d_q = nullptr; float* d_met = nullptr; float* d_llr = nullptr; float* d_saved = nullptr; Att* d_att = nullptr;
        int32_t* d_items = nullptr; int32_t* d_count = nullptr; int32_t* h_count = nullptr;
    } ft4coh;
    // FT4 weak search (ft8rx_ft4_set_weak, kernels/ft4_weak.hpp; allocated at the first FT4 batch that runs
    // with the setting on, WS_FT4_WEAK): the complex grid [max_frames][628][2306], the five mixes [5][576] and the 32 row turns
    struct Ft4Weak {
        bool on = false; float weak_min = FT8RX_FT4_WEAK_MIN_DEFAULT; size_t bytes = 0;
        cpx* d_cg = nullptr; cpx* d_mix = nullptr; cpx* d_rot = nullptr;
    } ft4weak;
    // FT4 OSD on the coherent rows (ft8rx_ft4_set_coh_osd, kernels/ft4_verify.hpp; allocated at the first FT4
    // batch that runs the step, WS_FT4_COSD).  Per candidate slot its position in the first failure list; per attempt (two per item of
    // OSD's list, at most 2 x max_frames << cand_shift) the gathered row, OSD's outcome, its NaN list and the score
    struct Ft4Cosd {
        bool on = false; float min_score = FT8RX_FT4_COH_OSD_MIN_SCORE_DEFAULT; int32_t max_hd = FT8RX_FT4_COH_OSD_MAX_HD_DEFAULT; size_t bytes = 0;
        int32_t* d_pos = nullptr; float* d_dense = nullptr; Att* d_att = nullptr; int32_t* d_nan = nullptr; float* d_score = nullptr;
    } ft4cosd;
    std::string err;
    bool profiling = false;
    std::vector<hipEvent_t> pev;
    std::vector<const char*> pnames;
    int n_stage = 0;
    float stage_ms[24] = {};
};
// a chunk index (BatchPlan::cb has MAX_CHUNKS + 1 boundaries) never leaves the per-chunk arrays: d_wcount, d_apc, d_apcount and
// d_rp_count are allocated with MAX_CHUNKS entries, and a stream index never leaves sub[] / ev_join[] / ev_cdone[][]
static_assert(sizeof(ft8rx_handle::ev_chunk) / sizeof(hipEvent_t) == batchplan::MAX_CHUNKS &&
              sizeof(ft8rx_handle::ap_chunk_version) / sizeof(uint32_t) == batchplan::MAX_CHUNKS &&
              sizeof(batchplan::BatchPlan::cb) / sizeof(int) == batchplan::MAX_CHUNKS + 1 &&
              batchplan::MAX_CHUNKS == 16 && batchplan::MAX_STREAMS == 8, "per-chunk arrays and the plan's boundaries");

// the streaming down-converter's index arithmetic (ddc_ring.hpp, host only) against the kernels' geometry
static_assert(ddcring::TILE == DDC_TO && ddcring::OUT_RING == 2 * FT8RX_NSAMP, "ddc_ring.hpp: tile and output ring");
static_assert(ddcframes::FT8_LEN == FT8RX_NSAMP && ddcframes::FT4_LEN == FT8RX_FT4_NSAMP, "ddc_frames.hpp: the two frame lengths");
template <int D> constexpr bool ddc_ring_geom_ok() {
    using G = DdcGeom<D>;
    return ddcring::geom(D).R1 == G::R1 && ddcring::geom(D).C1 == G::C1 && ddcring::geom(D).R2 == G::R2 && ddcring::geom(D).C2 == G::C2 &&
           ddcring::last(D) == (int64_t)(G::NV - 1 - G::C2) * G::R1 + G::C1 && ddcring::in_capacity(D) >= 12000 * D + ddcring::span(D);
}
static_assert(ddc_ring_geom_ok<1>() && ddc_ring_geom_ok<2>() && ddc_ring_geom_ok<4>() && ddc_ring_geom_ok<8>() && ddc_ring_geom_ok<16>(),
              "ddc_ring.hpp: the filter geometry is the kernels'");

// ... and of the spectrogram stage behind it (ddc_grid_ring.hpp) against k_grid_stream's: hop and window of spectrogram_hop, the output
// ring, two cycles of rows at the most; the hops of one launch (at most the grid ring's rows) advance less than one turn of the ring
static_assert(ddcgrid::HOP == 480 && ddcgrid::WIN == 3840 && ddcgrid::WIN == 2 * 1920 && ddcgrid::OUT_RING == ddcring::OUT_RING &&
              375 * ddcgrid::HOP == FT8RX_NSAMP && ddcgrid::MAX_ROWS == 2 * 375 && ddcgrid::MIN_ROWS >= 1 &&
              ddcgrid::HOP * ddcgrid::MAX_ROWS <= ddcgrid::OUT_RING && ddcgrid::WIN <= ddcgrid::OUT_RING, "ddc_grid_ring.hpp: k_grid_stream's geometry");

static void set_err(ft8rx_handle* h, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    if (h) h->err = buf; else g_create_err = buf;
}

// Streams are a PROCESS-WIDE pool per device, created once and never destroyed.  The HIP runtime maps every stream onto one of four
// hardware queues when it is created, and commands of streams that share a queue execute in submission order.  The streams of the
// first handle of a process get a queue each (main, copy, H2D, second chunk stream); a handle created after that one had been
// destroyed used to get another mapping, with both chunk streams of a batch on ONE queue -- no overlap between the two halves of a
// batch: 82.4 k -> 70.9 k frames/s on the 8192-frame shard (tools/r05_alloc_probe.py, profiles/r05_notes.md).  Handles of one process
// share the pool (more ordering between them, never less: every wait refers to an event recorded earlier in host order).
#include <mutex>
struct StreamPool { hipStream_t main = nullptr, copy = nullptr, h2d = nullptr, sub[8] = {}; };
static std::mutex g_pool_mu;
static StreamPool g_pool[64];
static hipStream_t pool_stream(int device, hipStream_t StreamPool::* which, bool blocking) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    StreamPool& P = g_pool[device & 63];
    if (!(P.*which)) {
        hipStream_t s = nullptr;
        if ((blocking ? hipStreamCreate(&s) : hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) return nullptr;
        P.*which = s;
    }
    return P.*which;
}
static hipStream_t pool_sub(int device, int i) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    StreamPool& P = g_pool[device & 63];
    if (!P.sub[i] && hipStreamCreateWithFlags(&P.sub[i], hipStreamNonBlocking) != hipSuccess) P.sub[i] = nullptr;
    return P.sub[i];
}

// f(std::true_type()) or f(std::false_type()): a run-time bool as a template argument of what f launches
template <class F> static void with_bool(bool b, F f) { if (b) f(std::true_type()); else f(std::false_type()); }

template <typename T> static int dalloc(ft8rx_handle* h, T** p, size_t n) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, n * sizeof(T));
    if (e != hipSuccess) { set_err(h, "hipMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e)); return -2; }
    h->allocs.push_back(q); *p = (T*)q; return 0;
}
// page-locked host memory; dev: also its device address (for kernels that write it directly)
template <typename T> static int halloc(ft8rx_handle* h, T** p, size_t n, T** dev = nullptr) {
    void *q = nullptr, *d = nullptr;
    hipError_t e = hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess && dev && (e = hipHostGetDevicePointer(&d, q, 0)) != hipSuccess) hipHostFree(q);
    if (e != hipSuccess) { set_err(h, "hipHostMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e)); return -2; }
    h->pinned.push_back(q); *p = (T*)q; if (dev) *dev = (T*)d; return 0;
}

// The workspaces that are created when something first needs them, one group per user.  First use is all or nothing: the members are
// allocated through dev() / host() and further steps (a table upload) run under FIRST_HIP; done() marks the group ready only if every
// step succeeded.  Otherwise it releases what the attempt allocated, takes it off the owner lists and nulls the members again: the
// handle is as it was before the call, and the next call attempts the whole group again.  Launch sites are reached only behind a
// ready group, so none sees a null member.
enum WsGroup { WS_STAGING, WS_STAGING2, WS_STAGING_F32, WS_STAGING2_F32, WS_MASK, WS_RECALL, WS_REPORTS, WS_PACKED, WS_SUB, WS_SUBD, WS_ONES, WS_DDC, WS_BLANK, WS_BLANK_IN, WS_PAN, WS_FT4, WS_FT4_SUB, WS_FT4_COH, WS_FT4_REPORT, WS_FT4_WEAK, WS_FT4_COSD };
struct FirstUse {
    ft8rx_handle* h; WsGroup g; size_t nd, nh; int rc = 0;
    std::vector<void**> members;
    FirstUse(ft8rx_handle* h_, WsGroup g_) : h(h_), g(g_), nd(h_->allocs.size()), nh(h_->pinned.size()) {}
    template <typename T> void dev(T** p, size_t n) { if (!rc && !(rc = dalloc(h, p, n))) members.push_back((void**)p); }
    template <typename T> void host(T** p, size_t n, T** d = nullptr) {
        if (rc || (rc = halloc(h, p, n, d))) return;
        members.push_back((void**)p); if (d) members.push_back((void**)d);
    }
    int done() {
        if (!rc) { h->ready |= 1u << g; return 0; }
        while (h->allocs.size() > nd) { hipFree(h->allocs.back()); h->allocs.pop_back(); }
        while (h->pinned.size() > nh) { hipHostFree(h->pinned.back()); h->pinned.pop_back(); }
        for (void** m : members) *m = nullptr;
        return -2;
    }
};
static bool ws_ready(const ft8rx_handle* h, WsGroup g) { return (h->ready >> g) & 1u; }
#define FIRST_HIP(F, x) do { if (!(F).rc) { hipError_t _e = (x); if (_e != hipSuccess) { set_err((F).h, "%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); (F).rc = -2; } } } while (0)

// The handle's own device audio buffer ([max_frames][180000] int16: staging of the host-pointer entry points, ft8rx_staging_audio) is
// allocated when something first asks for it: a caller that keeps its audio resident in HBM (ft8rx_enqueue_batch) never pays the
// 360 KB per frame.  (d_audio2: the second staging buffer of the pipelined host entry, batch_begin)
static int need_staging(ft8rx_handle* h, bool second = false) {
    const WsGroup g = second ? WS_STAGING2 : WS_STAGING;
    if (ws_ready(h, g)) return 0;
    FirstUse F(h, g);
    F.dev(second ? &h->d_audio2 : &h->d_audio, (size_t)h->max_frames * FT8RX_NSAMP);
    return F.done();
}
// ... and the float32 frames' ([max_frames][180000] float: staging of the _f32 entry points, ft8rx_staging_audio_f32), 720 KB per frame
static int need_staging_f32(ft8rx_handle* h, bool second = false) {
    const WsGroup g = second ? WS_STAGING2_F32 : WS_STAGING_F32;
    if (ws_ready(h, g)) return 0;
    FirstUse F(h, g);
    F.dev(second ? &h->d_audio2_f : &h->d_audio_f, (size_t)h->max_frames * FT8RX_NSAMP);
    return F.done();
}
// The frames of a batch: int16 (sb = 2) or float32 (sb = 4) samples, on the device or on the host.  Only the two
// kernels that read audio (launch_spectrogram, launch_cyc_a) and the copies look at sb.
struct Frames {
    const void* p; int sb;
    Frames at(size_t frame) const { return Frames{(const char*)p + frame * FT8RX_NSAMP * (size_t)sb, sb}; }
    size_t bytes(size_t n_frames) const { return n_frames * FT8RX_NSAMP * (size_t)sb; }
};
static int need_staging(ft8rx_handle* h, int sb, bool second) { return sb == 4 ? need_staging_f32(h, second) : need_staging(h, second); }
static void* staging_of(ft8rx_handle* h, int sb, bool second) {
    return sb == 4 ? (void*)(second ? h->d_audio2_f : h->d_audio_f) : (void*)(second ? h->d_audio2 : h->d_audio);
}

static void host_twiddle(int n, int count, std::vector<cpx>& w) {
    w.resize(count);
    for (int t = 0; t < count; t++) {
        double ang = (2.0 * M_PI * (double)t) / (double)n;
        w[t] = make_float2((float)cos(ang), (float)(-sin(ang)));
    }
}
template <typename T> static int upload(ft8rx_handle* h, const T** dst, const std::vector<T>& v) {
    T* p; if (dalloc(h, &p, v.size())) return -2;
    if (hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { set_err(h, "table upload failed"); return -2; }
    *dst = p; return 0;
}

// Device scratch of the stage entry points: bump allocation out of chunks the handle keeps (h->arena), so that after the first call
// of a given size ft8rx_ldpc / ft8rx_osd / ... allocate nothing (the reference-style function API in pyft8_amd/decoders.py calls
// them once per vector).  A Scratch object resets the arena when it goes out of scope; chunks are released by ft8rx_destroy.
struct Scratch {
    ft8rx_handle* h;
    ~Scratch() { for (auto& c : h->arena) c.used = 0; }
    void* raw(size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        if (!bytes) bytes = 256;
        for (auto& c : h->arena) if (c.cap - c.used >= bytes) { void* q = (char*)c.p + c.used; c.used += bytes; return q; }
        // miss: a new chunk, grown geometrically (twice the largest so far) so that a sequence of calls with growing n settles after
        // O(log n) allocations; chunks no call is using any more are released first instead of piling up until ft8rx_destroy
        size_t largest = 0;
        for (auto& c : h->arena) if (c.cap > largest) largest = c.cap;
        size_t cap = bytes > 2 * largest ? bytes : 2 * largest;
        if (cap < ((size_t)1 << 20)) cap = (size_t)1 << 20;
        for (size_t i = 0; i < h->arena.size();) {
            if (h->arena[i].used == 0) { hipFree(h->arena[i].p); h->arena.erase(h->arena.begin() + i); } else i++;
        }
        void* q = nullptr;
        if (hipMalloc(&q, cap) != hipSuccess) { if (cap == bytes || hipMalloc(&q, bytes) != hipSuccess) return nullptr; cap = bytes; }
        h->arena.push_back({q, cap, bytes});
        return q;
    }
    template <typename T> T* get(size_t n) { return (T*)raw(n * sizeof(T)); }
    template <typename T> T* put(const T* src, size_t n) { T* q = get<T>(n); if (q && hipMemcpy(q, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr; return q; }
};

// Everything that is not a pipelined batch (stage entry points, the synchronous host entry, subtraction, profiling passes) uses the
// handle's shared workspaces from the main stream; while the chunk streams run free (batch_submit) their work is not ordered
// against the main stream, so such calls first wait until the batches in flight are complete.
static int quiesce(ft8rx_handle* h, bool next_is_batch = false) {
    // the result copy of the last batch waits for every chunk stream (free-running batches) and still reads the slot's device
    // buffers on the copy stream after a plain one -- either way nothing of a batch is pending once the copy stream is idle.
    // A plain BATCH after a plain batch need not wait on the host at all: its kernels follow the previous ones on the main stream (the
    // sub-streams were joined into it), it writes the OTHER result slot, and that slot's previous copy is ordered by its ev_done --
    // so small pipelined batches (enqueue k + 1 while k's results travel) keep their overlap.
    if (h->free_running || (h->last_slot >= 0 && !next_is_batch)) HIPCHK(h, hipStreamSynchronize(h->copy_s));
    h->free_running = false;
    h->need_barrier = true;
    return 0;
}
#define ENTER(h) do { HIPCHK(h, hipSetDevice((h)->device)); { const int _q = quiesce(h); if (_q) return _q; } } while (0)

// a ladder kernel, or -- msg_types != 0 -- its _ext twin: the same kernel instantiated with the extended validity predicate
// (ft8_valid77_ext), which takes the type mask as one more argument; at 0 the code is unchanged
template <class K, class KX, class... A>
static void launch_mt(K k, KX kx, unsigned mt, int grid, hipStream_t s, A... a) {
    if (!mt) k<<<grid, 64, 0, s>>>(a...);
    else kx<<<grid, 64, 0, s>>>(a..., mt);
}

// The opt-in steps (optins.hpp): what counts as active, and the one refusal of a setter or consumer `who` of kind `which` that an
// active setting excludes.  Turning a setting off is never refused.
static unsigned active_optins(const ft8rx_handle* h) {
    using namespace optins;
    return (h->slots[0].pk_buf ? bit(PACKED) : 0) | (h->msg_types != 0 ? bit(MSG_TYPES) : 0) | (h->ap.np != 0 ? bit(AP_CALLS) : 0) |
           (h->rc_armed ? bit(RECALL) : 0) | (h->weak ? bit(WEAK) : 0) | (h->reports ? bit(REPORTS) : 0);
}
static int refuse_conflict(ft8rx_handle* h, const char* who, optins::Id which, const char* hint = "") {
    const int c = optins::conflict(active_optins(h), which);
    if (c < 0) return 0;
    set_err(h, "%s: not supported together with %s%s", who, optins::TABLE[c].name, hint);
    return -1;
}

extern "C" {

int ft8rx_default_config(ft8rx_config* c) {
    if (!c) return -1;
    c->sync_score_min = 85.0f; c->max_cands = 200; c->f0_lo = 32; c->f0_hi = 960; c->h0_lo = -37; c->h0_hi = 87;
    c->bp_nc0_a = 35; c->bp_iters_a = 5; c->bp_nc0_b = 90; c->bp_iters_b = 20; c->osd_single = 30; c->osd_double = 2;
    c->llr_sd_min = 5.0f;
    c->osd_triple = 0; c->osd_max_hd = 0;
    return 0;
}

int ft8rx_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
int ft8rx_device_pci_bus_id(int device, char* buf, int len) {
    if (!buf || len < 16) return -1;
    return hipDeviceGetPCIBusId(buf, len, device) == hipSuccess ? 0 : -2;
}
int ft8rx_build_info(int32_t* grid_cols, int32_t* spec_bins, int32_t* max_f0) {
    static_assert(NF0MAX >= FT8RX_GRID_COLS && NF0MAX >= FT8RX_MAX_F0, "per-f0 scratch stride");
    if (grid_cols) *grid_cols = FT8RX_GRID_COLS;
    if (spec_bins) *spec_bins = FT8RX_SPEC_BINS;
    if (max_f0) *max_f0 = FT8RX_MAX_F0;
    return 0;
}
int ft8rx_build_limits(int32_t* max_cands, int32_t* event_cap) {
    static_assert(FT8RX_MAX_CANDS <= NF0MAX && (1 << cand_shift(FT8RX_MAX_CANDS)) == FT8RX_MAX_CANDS,
                  "max_cands: never more than k_topk has keys, and the largest candidate stride is the limit itself");
    if (max_cands) *max_cands = FT8RX_MAX_CANDS;
    if (event_cap) *event_cap = FT8RX_EVENT_CAP;
    return 0;
}

int ft8rx_get_fft_plans(int32_t* p1920, int32_t* p3200, int32_t* p300, int32_t* p320) {
    const int32_t a[8] = {8, 4, 4, 5, 3, 0, 0, 0}, b[8] = {8, 4, 4, 5, 5, 0, 0, 0}, c[8] = {5, 5, 4, 3, 0, 0, 0, 0}, d[8] = {8, 8, 5, 0, 0, 0, 0, 0};
    if (p1920) memcpy(p1920, a, sizeof(a));
    if (p3200) memcpy(p3200, b, sizeof(b));
    if (p300) memcpy(p300, c, sizeof(c));
    if (p320) memcpy(p320, d, sizeof(d));
    return 0;
}

const char* ft8rx_last_error(ft8rx_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

void ft8rx_destroy(ft8rx_handle* h) {
    if (!h) return;
    hipSetDevice(h->device);
    // the streams belong to the process-wide pool and stay: wait for everything this handle has put on them, then free its memory
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->copy_s) hipStreamSynchronize(h->copy_s);
    if (h->h2d_s) hipStreamSynchronize(h->h2d_s);
    for (int i = 0; i < 8; i++) { if (h->sub[i]) hipStreamSynchronize(h->sub[i]); if (h->ev_join[i]) hipEventDestroy(h->ev_join[i]); }
    for (void* p : h->allocs) hipFree(p);
    for (auto& c : h->arena) hipFree(c.p);
    for (auto e : h->pev) hipEventDestroy(e);
    for (int k = 0; k < 2; k++) for (int i = 0; i < 8; i++) if (h->ev_cdone[k][i]) hipEventDestroy(h->ev_cdone[k][i]);
    for (int i = 0; i < 32; i++) if (h->d2h_ev[i]) hipEventDestroy(h->d2h_ev[i]);
    for (hipEvent_t e : h->ev_chunk) if (e) hipEventDestroy(e);
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ddc_ev) hipEventDestroy(h->ddc_ev);
    if (h->ds.ev) hipEventDestroy(h->ds.ev);
    if (h->ps.ev) hipEventDestroy(h->ps.ev);
    if (h->bis.ev) hipEventDestroy(h->bis.ev);
    if (h->pans.ev) hipEventDestroy(h->pans.ev);
    for (ResultSlot& sl : h->slots) {
        if (sl.ev_comp) hipEventDestroy(sl.ev_comp);
        if (sl.ev_done) hipEventDestroy(sl.ev_done);
    }
    for (void* p : h->pinned) hipHostFree(p);
    delete h;
}

int ft8rx_create(const ft8rx_config* cfg, int device, int max_frames, ft8rx_handle** out) {
    if (!cfg || !out || max_frames < 1) { set_err(nullptr, "ft8rx_create: bad arguments"); return -1; }
    if (cfg->max_cands < 1 || cfg->max_cands > FT8RX_MAX_CANDS || cfg->f0_lo < 4 || cfg->f0_hi > FT8RX_MAX_F0 || cfg->f0_lo >= cfg->f0_hi ||
        cfg->h0_hi <= cfg->h0_lo || cfg->h0_lo < FT8RX_MIN_H0 || cfg->h0_hi > FT8RX_MAX_H0 || cfg->bp_nc0_a > cfg->bp_nc0_b || cfg->bp_iters_a > cfg->bp_iters_b ||
        cfg->osd_single < 0 || cfg->osd_single > OSD_MAXFLIP || cfg->osd_double < 0 || cfg->osd_double > OSD_MAXFLIP ||
        cfg->osd_triple < 0 || cfg->osd_triple > 40 || cfg->osd_max_hd < 0 || cfg->osd_max_hd > 174 ||
        osd_trial_table(cfg->osd_single, cfg->osd_double, cfg->osd_triple).size() > OSD_MAXTRIALS) {
        set_err(nullptr, "ft8rx_create: configuration out of the supported range"); return -1; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_err(nullptr, "ft8rx_create: no HIP device available (this library has no CPU fallback)"); return -3; }
    if (device < 0 || device >= ndev) { set_err(nullptr, "ft8rx_create: device %d out of range (%d devices)", device, ndev); return -1; }
    ft8rx_handle* h = new ft8rx_handle();
    h->cfg = *cfg; h->device = device; h->max_frames = max_frames;
    if (hipSetDevice(device) != hipSuccess || !(h->stream = pool_stream(device, &StreamPool::main, true))) { set_err(nullptr, "ft8rx_create: cannot open device %d", device); delete h; return -2; }
    const size_t B = (size_t)max_frames, S = (size_t)1 << cand_shift(*cfg);      // S: per-frame stride of the per-candidate workspaces
    int rc = 0;
    rc |= dalloc(h, &h->d_grid, B * FT8RX_GRID_ROWS * FT8RX_GRID_COLS);
    rc |= dalloc(h, &h->d_best_score, B * NF0MAX);
    rc |= dalloc(h, &h->d_best_h0, B * NF0MAX);
    rc |= dalloc(h, &h->d_rec, B * S);
    rc |= dalloc(h, &h->d_ncand, B);
    rc |= dalloc(h, &h->d_llr0, B * S * 174);
    rc |= dalloc(h, &h->d_saved, B * S * 5 * 174);
    rc |= dalloc(h, &h->d_att0, B * S * 5);
    rc |= dalloc(h, &h->d_attG, B * S * 2);
    rc |= dalloc(h, &h->d_attB, B * S * 5);
    rc |= dalloc(h, &h->d_attO, B * S * 10);
    // The four-step scratch (768 KB per frame) and the cycle spectrum (393 KB; 768 KB in the wide build) live INSIDE the grid buffer: the
    // dB grid is dead once k_grid_llr has gathered the payloads, and the cycle FFT only starts after that (enqueue_chain places a chunk's
    // A and spectrum at the start of the chunk's own grid region; k_spectrogram rewrites the constant row 0 with every batch).  The
    // stage entry points use one of the three at a time.  -1.16 MB of HBM per frame.
    static_assert((size_t)(96000 + FT8RX_SPEC_BINS) * sizeof(cpx) <= (size_t)FT8RX_GRID_ROWS * FT8RX_GRID_COLS * sizeof(float), "scratch A + cycle spectrum fit a frame's grid");
    if (!rc) { h->d_A = reinterpret_cast<cpx*>(h->d_grid); h->d_spec = h->d_A + B * 96000; }
    for (int i = 0; i < WL_N; i++) rc |= dalloc(h, &h->d_work[i], B * S * WL_MULT(i));      // WL_BP0 / WL_OSDNAN list attempts
    rc |= dalloc(h, &h->d_wcount, (size_t)batchplan::MAX_CHUNKS * WL_N);
    rc |= dalloc(h, &h->d_apc, batchplan::MAX_CHUNKS);       // ft8rx_set_ap_calls allocates nothing: it is called every cycle
    rc |= dalloc(h, &h->d_apcount, (size_t)batchplan::MAX_CHUNKS * 2);
    rc |= dalloc(h, &h->d_ev, B * FT8RX_EVENT_CAP);
    rc |= dalloc(h, &h->d_evcount, B);
    ResultSlot* const sl = h->slots;
    sl[0].rec = h->d_rec; sl[0].ncand = h->d_ncand; sl[0].ev = h->d_ev; sl[0].evcount = h->d_evcount;
    rc |= dalloc(h, &sl[1].rec, B * S);
    rc |= dalloc(h, &sl[1].ncand, B);
    rc |= dalloc(h, &sl[1].ev, B * FT8RX_EVENT_CAP);
    rc |= dalloc(h, &sl[1].evcount, B);
    const bool ev_compact = B * FT8RX_EVENT_CAP * sizeof(ft8rx_event) > EV_EAGER_BYTES;
    for (int k = 0; k < 2 && ev_compact; k++) rc |= dalloc(h, &sl[k].d_evoffs, B + 1);
    for (int k = 0; k < 2 && !rc; k++) {
        rc = halloc(h, &sl[k].h_rec, B * cfg->max_cands);
        if (!rc) rc = halloc(h, &sl[k].h_cnt, B);
        if (!rc) rc = halloc(h, &sl[k].h_ev, B * FT8RX_EVENT_CAP);
        if (!rc) rc = halloc(h, &sl[k].h_evc, B);
        if (!rc && ev_compact) rc = halloc(h, &sl[k].h_evpacked, B * FT8RX_EVENT_CAP, &sl[k].d_evpacked);
    }
    if (rc) { g_create_err = h->err; ft8rx_destroy(h); return -2; }
    // ---- tables (double precision on the host, rounded once)
    std::vector<float> win(3840);
    for (int i = 0; i < 3840; i++) win[i] = (float)(0.5 + 0.5 * cos(M_PI * (double)(2 * i + 1 - 3840) / 3839.0));   // np.hanning (receiver.py:236)
    std::vector<double> taper(100);
    { double step = (0.0 - M_PI) / 99.0; for (int i = 0; i < 100; i++) { double y = (i == 99) ? 0.0 : (double)i * step + M_PI; taper[i] = 0.5 * (1.0 + cos(y)); } }   // receiver.py:183-184
    std::vector<cpx> w;
    rc |= upload(h, &h->T.win, win);
    rc |= upload(h, &h->T.taper, taper);
    host_twiddle(1920, 1920, w);   rc |= upload(h, &h->T.W1920, w);
    host_twiddle(3840, FT8RX_GRID_COLS, w);    rc |= upload(h, &h->T.WR3840, w);
    host_twiddle(3200, 3200, w);   rc |= upload(h, &h->T.W3200, w);
    host_twiddle(96000, 96000, w); rc |= upload(h, &h->T.W96000, w);
    host_twiddle(300, 300, w);     rc |= upload(h, &h->T.W300, w);
    host_twiddle(320, 320, w);     rc |= upload(h, &h->T.W320, w);
    host_twiddle(192000, FT8RX_SPEC_BINS, w); rc |= upload(h, &h->T.WR192k, w);
    host_twiddle(32, 32, w);       rc |= upload(h, &h->T.W32, w);
    {   // tables of the frequency-domain fine score (kernels/fine_sync.hpp: fine_fscore; oracle/ft8_oracle.c: make_fscore_tables -- same formulas)
        std::vector<float> k32(1800);
        std::vector<cpx> cs(156), g1000(1000);
        for (int m = -900; m < 900; m++) {
            const int r = ((m % 100) + 100) % 100;
            k32[m + 900] = (r == 0) ? (m == 0 ? 32.0f : 0.0f) : (float)(sin(M_PI * (double)r / 100.0) / sin(M_PI * (double)m / 3200.0));
        }
        for (int sidx = 1; sidx < 7; sidx++) for (int q = 0; q <= 25; q++) {
            const double a = 2.0 * M_PI * (double)((q * sidx) % 100) / 100.0;
            cpx v = make_float2((float)cos(a), (float)sin(a));
            if (q == 0) v = make_float2(1.0f, 0.0f);
            cs[(sidx - 1) * 26 + q] = v;
        }
        for (int k = -150; k < 850; k++) {
            const int r = ((k % 100) + 100) % 100, j = (k - r) / 100;
            const double a = M_PI * (31.0 * (double)r - 100.0 * (double)j) / 3200.0;
            g1000[k + 150] = make_float2((float)cos(a), (float)sin(a));
        }
        std::vector<cpx> tw100(100);
        for (int m = 0; m < 100; m++) { const double a = -2.0 * M_PI * (double)m / 100.0; tw100[m] = make_float2((float)cos(a), (float)sin(a)); }
        rc |= upload(h, &h->T.K32, k32); rc |= upload(h, &h->T.CS100, cs); rc |= upload(h, &h->T.G1000, g1000); rc |= upload(h, &h->T.TW100, tw100);
    }
    if (rc) { g_create_err = h->err; ft8rx_destroy(h); return -2; }
    // LDPC tables
    bool ok = true;
    ok &= hipMemcpyToSymbol(HIP_SYMBOL(d_CHK_N), FT8_CHK_N, sizeof(FT8_CHK_N)) == hipSuccess;
    ok &= hipMemcpyToSymbol(HIP_SYMBOL(d_CHK_V), FT8_CHK_V, sizeof(FT8_CHK_V)) == hipSuccess;
    {   // k_bp's edge slots, renumbered slot-major (round 6): edge j of check c lives at 83 j + c (j < 6), the seventh edge of the 24
        // degree-7 checks (c >= 59) at 498 + (c - 59).  The check-parallel products then read CONSECUTIVE words, tl[c + 83 j] -- with
        // the generated row-major numbering (check c's edges at 6 c .. 6 c + 5) lane c read word 6 c + j: 16 banks, four lanes each.
        // Only the names of the slots change: products still run over j ascending, a variable's three deltas are still added in
        // the order of FT8_VAR_E (ascending ROW-MAJOR edge number = np.add.at's order, decoders.py:150).
        static uint8_t ev[522], ec[522]; static uint16_t ve[174][3];
        auto slot = [](int e) { const int c = FT8_EDGE_C[e], j = e - FT8_CHK_E0[c]; return j < 6 ? 83 * j + c : 498 + (c - 59); };
        for (int e = 0; e < 522; e++) { ev[slot(e)] = FT8_EDGE_V[e]; ec[slot(e)] = FT8_EDGE_C[e]; }
        for (int v = 0; v < 174; v++) for (int k = 0; k < 3; k++) ve[v][k] = (uint16_t)slot(FT8_VAR_E[v][k]);
        ok &= hipMemcpyToSymbol(HIP_SYMBOL(d_EDGE_V), ev, sizeof(ev)) == hipSuccess;
        ok &= hipMemcpyToSymbol(HIP_SYMBOL(d_EDGE_C), ec, sizeof(ec)) == hipSuccess;
        ok &= hipMemcpyToSymbol(HIP_SYMBOL(d_VAR_E), ve, sizeof(ve)) == hipSuccess;
    }
    ok &= hipMemcpyToSymbol(HIP_SYMBOL(d_G0), FT8_G0, sizeof(FT8_G0)) == hipSuccess;
    {   // recall's parity columns (kernels/recall.hpp: d_RCG): parity bit 91 + j of the systematic generator
        static uint64_t rcg[83][2];
        memset(rcg, 0, sizeof(rcg));
        for (int r = 0; r < 91; r++) for (int j = 0; j < 83; j++) {
            const int v = 91 + j;
            if ((FT8_G0[r][v >> 6] >> (v & 63)) & 1ull) rcg[j][r >> 6] |= 1ull << (r & 63);
        }
        ok &= hipMemcpyToSymbol(HIP_SYMBOL(d_RCG), rcg, sizeof(rcg)) == hipSuccess;
    }
    {   // per-check membership masks (3 x 64 bits), so a lane gets its two checks' masks with 6 coalesced loads
        static uint64_t cm[128][3];
        memset(cm, 0, sizeof(cm));
        for (int c = 0; c < 83; c++) for (int j = 0; j < FT8_CHK_N[c]; j++) { int v = FT8_CHK_V[c][j]; cm[c][v >> 6] |= 1ull << (v & 63); }
        ok &= hipMemcpyToSymbol(HIP_SYMBOL(d_CHK_MASK), cm, sizeof(cm)) == hipSuccess;
    }
    {   // CRC-14 syndromes of the 77 unit messages (bit-serial definition, decoders.py:123-129)
        uint16_t syn[77];
        for (int pos = 0; pos < 77; pos++) syn[pos] = (uint16_t)hostmsg::crc14_serial(pos < 64 ? (1ull << pos) : 0ull, pos >= 64 ? (1ull << (pos - 64)) : 0ull);
        ok &= hipMemcpyToSymbol(HIP_SYMBOL(d_CRC_SYN), syn, sizeof(syn)) == hipSuccess;
    }
    {   // OSD: G0 column-wise (91 row bits per column) and the byte-wise CRC syndrome table of the 91-bit word
        static uint32_t g0t[192][3];
        memset(g0t, 0, sizeof(g0t));
        for (int r = 0; r < 91; r++) for (int v = 0; v < 174; v++) if ((FT8_G0[r][v >> 6] >> (v & 63)) & 1ull) g0t[v][r >> 5] |= 1u << (r & 31);
        ok &= hipMemcpyToSymbol(HIP_SYMBOL(d_G0T), g0t, sizeof(g0t)) == hipSuccess;
        uint16_t syn91[96]; memset(syn91, 0, sizeof(syn91));
        for (int v = 0; v < 91; v++) {
            if (v < 77) { const int pos = 76 - v; syn91[v] = (uint16_t)hostmsg::crc14_serial(pos < 64 ? (1ull << pos) : 0ull, pos >= 64 ? (1ull << (pos - 64)) : 0ull); }
            else syn91[v] = (uint16_t)(1u << (13 - (v - 77)));
        }
        uint32_t synm[14][3]; memset(synm, 0, sizeof(synm));
        for (int v = 0; v < 91; v++) for (int k = 0; k < 14; k++) if ((syn91[v] >> k) & 1) synm[k][v >> 5] |= 1u << (v & 31);
        ok &= hipMemcpyToSymbol(HIP_SYMBOL(d_SYNM), synm, sizeof(synm)) == hipSuccess;
        static uint16_t ct[12][256];
        for (int b = 0; b < 12; b++) for (int x = 0; x < 256; x++) { uint16_t a = 0; for (int t = 0; t < 8; t++) if ((x >> t) & 1) a ^= syn91[8 * b + t]; ct[b][x] = a; }
        ok &= hipMemcpyToSymbol(HIP_SYMBOL(d_CRC_T), ct, sizeof(ct)) == hipSuccess;
        {   // np.argsort of an all-NaN vector (kernels/osd.hpp: d_NANPERM)
            float xn[174]; int perm[176], stk[64]; uint8_t p8[192];
            for (int i = 0; i < 174; i++) xn[i] = NAN;
            osd_std_sort_withnan(xn, perm, stk);
            memset(p8, 0, sizeof(p8));
            for (int i = 0; i < 174; i++) p8[i] = (uint8_t)perm[i];
            ok &= hipMemcpyToSymbol(HIP_SYMBOL(d_NANPERM), p8, sizeof(p8)) == hipSuccess;
        }
        const std::vector<uint32_t> tr = osd_trial_table(cfg->osd_single, cfg->osd_double, cfg->osd_triple);
        h->n_trials = (int)tr.size();
        if (upload(h, &h->d_trials, tr)) ok = false;
    }
    if (!ok) { set_err(nullptr, "ft8rx_create: device table upload failed"); ft8rx_destroy(h); return -2; }
    if (sync_lds_bytes(*cfg) > 65536) {
        ok &= hipFuncSetAttribute((const void*)k_sync, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sync_lds_bytes(*cfg)) == hipSuccess;
        ok &= hipFuncSetAttribute((const void*)k_sync_acc, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sync_lds_bytes(*cfg)) == hipSuccess;
    }
    if (!ok) { set_err(nullptr, "ft8rx_create: cannot reserve LDS for k_sync"); ft8rx_destroy(h); return -2; }
    // the never-written grid row 0 (receiver.py:240)
    int nfill = (int)B * FT8RX_GRID_COLS;
    k_fill_row0<<<(nfill + 255) / 256, 256, 0, h->stream>>>(h->d_grid, (int)B);
    if (hipStreamSynchronize(h->stream) != hipSuccess) { set_err(nullptr, "ft8rx_create: init kernel failed"); ft8rx_destroy(h); return -2; }
    bool okc = true;
    for (int i = 0; i < 24; i++) { hipEvent_t e = nullptr; okc = okc && hipEventCreate(&e) == hipSuccess; if (e) h->pev.push_back(e); }
    // (the chunk streams h->sub[] are created on first use, batch_begin: every stream that exists competes for one of the
    // runtime's four hardware queues, see the note in batch_plan.hpp)
    // (measurement aid: FT8RX_SUBS_FIRST=n creates n chunk streams BEFORE the copy streams, i.e. gives them hardware queues of their own
    // -- for A/B runs of three or four chunk streams, profiles/r06_notes.md)
    if (const char* e = getenv("FT8RX_SUBS_FIRST")) for (int i = 0; i < atoi(e) && i < 8; i++) pool_sub(device, i);
    okc = okc && (h->copy_s = pool_stream(device, &StreamPool::copy, false)) != nullptr;
    okc = okc && (h->h2d_s = pool_stream(device, &StreamPool::h2d, false)) != nullptr;
    for (hipEvent_t& e : h->ev_chunk) okc = okc && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    okc = okc && hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) == hipSuccess;
    for (ResultSlot& s : h->slots) {
        okc = okc && hipEventCreateWithFlags(&s.ev_comp, hipEventDisableTiming) == hipSuccess;
        okc = okc && hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming) == hipSuccess;
    }
    if (!okc) { set_err(nullptr, "ft8rx_create: cannot create HIP streams/events"); ft8rx_destroy(h); return -2; }
    *out = h;
    return 0;
}

int ft8rx_set_profiling(ft8rx_handle* h, int on) { if (!h) return -1; h->profiling = on != 0; return 0; }

int ft8rx_get_stage_times(ft8rx_handle* h, int* n, const char** names, float* ms) {
    if (!h || !n) return -1;
    *n = h->n_stage;
    for (int i = 0; i < h->n_stage; i++) { if (names) names[i] = h->pnames[i]; if (ms) ms[i] = h->stage_ms[i]; }
    return 0;
}


// the kernel chain for frames [f0, f0+B) on stream s (all buffers are frame-major, so a chunk is a pointer offset)
// ladder kernels launch a bounded grid that strides over their work list (a few items per block at most): enough blocks to fill the
// chip four times over (LADDER_GRID_CAP; ft8rx_set_ladder_grid lowers the handle's cap), never more than there can be items
static int ladder_grid(const ft8rx_handle* h, int max_items) { return max_items < h->ladder_cap ? max_items : h->ladder_cap; }

// the sync search of frames [.., B) over the configured h0 range, in windows of SYNC_WIN offsets (one launch for any range up to 14 s):
// the first window's kernel sets the best score per f0, the later windows' one accumulates into it.  Weak mode (ft8rx_set_weak): the
// three-block score, in windows of SYNC3_WIN offsets
static void launch_sync(const float* grid, float* bs, int32_t* bh, const ft8rx_config& c, int B, hipStream_t s, bool weak) {
    const auto first = weak ? k_sync3 : k_sync, acc = weak ? k_sync3_acc : k_sync_acc;
    const int win = weak ? SYNC3_WIN : SYNC_WIN;
    const size_t lds = weak ? 0 : sync_lds_bytes(c);
    const int ntile = (c.f0_hi - c.f0_lo + 15) / 16;
    for (int lo = c.h0_lo; lo < c.h0_hi; lo += win) {
        ft8rx_config w = c;
        w.h0_lo = lo; w.h0_hi = lo + win < c.h0_hi ? lo + win : c.h0_hi;
        (lo == c.h0_lo ? first : acc)<<<dim3(ntile, B), 256, lds, s>>>(grid, bs, bh, w);
    }
}
// The configuration the existing kernels see in weak mode: the weak sync threshold (k_topk), no sd stop at grid or fine
// (k_grid_llr, k_fine_weak), and the OSD distance gate -- an explicit config.osd_max_hd wins over the setting's
static ft8rx_config weak_config(const ft8rx_handle* h) {
    ft8rx_config w = h->cfg;
    w.sync_score_min = h->weak_sync_min;
    w.llr_sd_min = -INFINITY;
    if (!w.osd_max_hd) w.osd_max_hd = h->weak_osd_max_hd;
    return w;
}
// the fine sync of n_blocks work-list blocks or test triples: weak mode's kernel, or k_fine plus -- need_td -- k_fine_td for the
// candidates beyond the frequency-domain h0 range (-6.1 .. +8.3 s) that k_fine leaves out
static void launch_fine(ft8rx_handle* h, const ft8rx_config& cfg, bool weak, int n_blocks, hipStream_t s, const cpx* spec, ft8rx_record* rec,
                        const int32_t* ncand, float* llr, const int32_t* trip, int32_t* t_out, float* t_sd, float* t_sgrid, WorkList work,
                        bool need_td) {
    if (weak) { k_fine_weak<<<n_blocks, FINE_NT, 0, s>>>(spec, rec, ncand, llr, h->T, cfg, trip, t_out, t_sd, t_sgrid, work); return; }
    ft8rx_ilp_fine(n_blocks, s, spec, rec, ncand, llr, h->T, cfg, trip, t_out, t_sd, t_sgrid, work);
    if (need_td) k_fine_td<<<n_blocks, FINE_NT, 0, s>>>(spec, rec, ncand, llr, h->T, cfg, trip, t_out, t_sd, t_sgrid, work);
}

// OSD of `grid` blocks -- mode 0: striding over `work` x 10 attempts, mode 2: one raw vector each -- then of the attempts they left on `nanl`: vectors
// with a NaN (a NaN-poisoned BP output), which the reference's numpy orders with std::sort -- a kernel of their own, of OSD_NAN_GRID blocks
// or the handle's cap (ft8rx_set_ladder_grid), in either mode: it strides over a list.  osd_wide: kernels/osd.hpp
static bool osd_wide(int nflip) { return nflip > OSD_FLIPS_A; }
static void launch_osd(const ft8rx_handle* h, unsigned mt, int grid, hipStream_t s, int mode, const float* llr, const float* saved, const Att* attB, ft8rx_record* rec,
                       const int32_t* ncand, Att* attO, ft8rx_event* ev, int32_t* evc, const uint32_t* trials, int ntr, int nflip, int max_hd,
                       int sh, WorkList work, WorkList nanl) {
    const bool wide = osd_wide(nflip);
    launch_mt(wide ? k_osd_wide : k_osd, wide ? k_osd_wide_ext : k_osd_ext, mt, grid, s,
              mode, llr, saved, attB, rec, ncand, attO, ev, evc, trials, ntr, nflip, max_hd, sh, work, nanl);
    launch_mt(wide ? k_osd_nan_wide : k_osd_nan, wide ? k_osd_nan_wide_ext : k_osd_nan_ext, mt, ladder_grid(h, OSD_NAN_GRID), s,
              mode, llr, saved, attB, rec, ncand, attO, ev, evc, trials, ntr, nflip, max_hd, sh, nanl);
}

// ipass 7 of B frames (kernels/ap_calls.hpp): candidate list in cand_items (B * stride entries), OSD list in osd_items (B * stride * 3),
// attempt results in attO (B * stride * 10), the two list counters at ac; the batch chain and ft8rx_ap_calls_probe launch the same
static void launch_ap_calls(ft8rx_handle* h, int B, const float* llr0, ft8rx_record* rec, const int32_t* ncand, Att* attO, ft8rx_event* ev,
                            int32_t* evc, int32_t* cand_items, int32_t* osd_items, int32_t* ac, const ApCalls* apc, hipStream_t s) {
    const ft8rx_config& c = h->cfg;
    const int sh = cand_shift(c); const size_t S = (size_t)1 << sh;
    const int nflip = osd_nflip(c.osd_single, c.osd_triple);
    hipMemsetAsync(ac, 0, 2 * sizeof(int32_t), s);
    const WorkList cl = {cand_items, ac}, ol = {osd_items, ac + 1};
    k_ap_worklist<<<(B * S + 255) / 256, 256, 0, s>>>(rec, ncand, B, sh, cl);
    k_bp_ap<<<ladder_grid(h, B * c.max_cands * h->ap.np), 64, 0, s>>>(llr0, rec, ncand, attO, ev, evc, c, apc, cl, ol);
    (osd_wide(nflip) ? k_osd_ap_wide : k_osd_ap)<<<ladder_grid(h, B * c.max_cands * 3), 64, 0, s>>>(
        llr0, rec, ncand, attO, ev, evc, h->d_trials, h->n_trials, nflip, sh, apc, ol);
    k_select_ap<<<(B * S + 255) / 256, 256, 0, s>>>(rec, attO, apc, cl);
}

// the measurement step of B frames (kernels/report.hpp): the DECODED slots of rec -> items / *count, their reports -> rep (indexed like
// rec); the batch chain and ft8rx_report_probe launch the same
static void launch_reports(ft8rx_handle* h, int B, const cpx* spec, const ft8rx_record* rec, const int32_t* ncand, int32_t* items,
                           int32_t* count, ft8rx_report* rep, hipStream_t s) {
    const ft8rx_config& c = h->cfg;
    const int sh = cand_shift(c); const size_t S = (size_t)1 << sh;
    hipMemsetAsync(count, 0, sizeof(int32_t), s);
    const WorkList wl = {items, count};
    k_report_worklist<<<(B * S + 255) / 256, 256, 0, s>>>(rec, ncand, B, sh, wl, rep);
    k_report<<<ladder_grid(h, B * c.max_cands), FINE_NT, 0, s>>>(spec, rec, rep, h->T, sh, wl);
}

// the two kernels of the chain that read audio, in the form of the frames' samples (B frames from a.p on)
static void launch_spectrogram(int B, hipStream_t s, const Frames& a, float* grid, const Tables& T) {
    if (a.sb == 4) k_spectrogram_f32<<<dim3(376, B), SPEC_NT, 0, s>>>((const float*)a.p, grid, T);
    else ft8rx_ilp_spectrogram(B, s, (const int16_t*)a.p, grid, T);
}
static void launch_cyc_a(int B, hipStream_t s, const Frames& a, cpx* A, const Tables& T) {
    if (a.sb == 4) k_cyc_a_f32<<<dim3(40, B), 256, 0, s>>>((const float*)a.p, A, T);
    else k_cyc_a<<<dim3(40, B), 256, 0, s>>>((const int16_t*)a.p, A, T);
}

static void enqueue_chain(ft8rx_handle* h, const Frames& d_audio, int f0, int B, hipStream_t s, bool prof, int slot, int chunk) {
    const ResultSlot& sl = h->slots[slot];
    const bool weak = h->weak;                                     // the setting this batch was enqueued with
    const ft8rx_config cw = weak ? weak_config(h) : h->cfg;
    const ft8rx_config& c = weak ? cw : h->cfg;
    const size_t F = (size_t)f0;
    const int sh = cand_shift(c); const size_t S = (size_t)1 << sh, FS = F * S;        // candidate stride (ft8rx_create)
    const Frames audio = d_audio.at(F);
    float* grid = h->d_grid + F * FT8RX_GRID_ROWS * FT8RX_GRID_COLS;
    float* bs = h->d_best_score + F * NF0MAX; int32_t* bh = h->d_best_h0 + F * NF0MAX;
    ft8rx_record* rec = sl.rec + FS; int32_t* ncand = sl.ncand + F;
    float* llr0 = h->d_llr0 + FS * 174; float* saved = h->d_saved + FS * 5 * 174;
    Att* att0 = h->d_att0 + FS * 5; Att* attG = h->d_attG + FS * 2; Att* attB = h->d_attB + FS * 5; Att* attO = h->d_attO + FS * 10;
    cpx* A = reinterpret_cast<cpx*>(grid); cpx* spec = A + (size_t)B * 96000;      // inside this chunk's (by then dead) grid region, see ft8rx_create
    ft8rx_event* ev = sl.ev + F * FT8RX_EVENT_CAP; int32_t* evc = sl.evcount + F;
#define STAGE(name) do { if (prof) { hipEventRecord(h->pev[h->pnames.size()], s); h->pnames.push_back(name); } } while (0)
    int32_t* wc = h->d_wcount + WL_N * chunk;                      // (evc and wc are zeroed by k_topk)
    WorkList wl[WL_N];
    for (int i = 0; i < WL_N; i++) { wl[i].items = h->d_work[i] + FS * WL_MULT(i); wl[i].count = wc + i; }
    STAGE("spectrogram");
    launch_spectrogram(B, s, audio, grid, h->T);
    STAGE("sync");
    launch_sync(grid, bs, bh, c, B, s, weak);
    STAGE("topk");
    k_topk<<<B, 1024, 0, s>>>(bs, bh, rec, ncand, c, evc, wc, h->use_mask ? h->d_colmask + F * NF0MAX : nullptr);
    STAGE("grid_llr");
    const unsigned mt = (unsigned)h->msg_types;                    // (launch_mt)
    launch_mt(k_grid_llr, k_grid_llr_ext, mt, XCD_GRID(B, c.max_cands), s, grid, rec, ncand, llr0, c, nullptr, nullptr, nullptr, att0, ev, evc, B);
    k_worklist_att<<<(B * S * 5 + 255) / 256, 256, 0, s>>>(rec, ncand, att0, B, sh, wl[WL_BP0]);
    STAGE("bp_grid");
    launch_mt(k_bp, k_bp_ext, mt, ladder_grid(h, B * c.max_cands * 5), s, 0, llr0, rec, ncand, nullptr, att0, nullptr, ev, evc, c, c.bp_nc0_a, c.bp_iters_a, wl[WL_BP0], 0, 5);
    STAGE("select0");
    k_select0<<<(B * S + 255) / 256, 256, 0, s>>>(rec, ncand, att0, B, sh, wl[WL_FINE]);
    STAGE("cycle_fft");
    launch_cyc_a(B, s, audio, A, h->T);
    k_cyc_bc<<<dim3(CYC_BC_GRID, B), 256, 0, s>>>(A, spec, h->T);
    STAGE("fine");
    launch_fine(h, c, weak, ladder_grid(h, B * c.max_cands), s, spec, rec, ncand, llr0, nullptr, nullptr, nullptr, nullptr, wl[WL_FINE],
                c.h0_lo < FT8RX_MIN_H0_FD || c.h0_hi > FT8RX_MAX_H0_FD + 1);      // a search_time_range beyond -6.1 .. +8.3 s
    k_worklist<<<(B * S + 255) / 256, 256, 0, s>>>(rec, ncand, B, sh, wl[WL_BP1]);
    STAGE("bp_fine");
    // fine-stage BP: in ladder order (three launches; decided candidates drop out), or -- ft8rx_set_ladder_mode(h, 1), for small
    // batches where latency matters more than work -- all five variants in one launch: one dependent BP instead of three, same
    // records and messages (the event log then also holds entries of attempts the ladder would not have reached)
    const auto bp_fine = [&](int n_variants, const WorkList& work, int v0) {      // variants v0 .. v0 + n_variants - 1 of the items of `work`
        launch_mt(k_bp, k_bp_ext, mt, B * c.max_cands * n_variants, s, 1, llr0, rec, ncand, attG, attB, saved, ev, evc, c, c.bp_nc0_b, c.bp_iters_b,
                  work, v0, n_variants);
    };
    if (h->ladder_mode == 0) {
        bp_fine(1, wl[WL_BP1], 0);
        k_select1<<<(B * S + 255) / 256, 256, 0, s>>>(0, rec, ncand, attG, attB, B, c, wl[WL_BP1B]);
        bp_fine(1, wl[WL_BP1B], 1);
        k_select1<<<(B * S + 255) / 256, 256, 0, s>>>(1, rec, ncand, attG, attB, B, c, wl[WL_BP1C]);
        bp_fine(3, wl[WL_BP1C], 2);
        STAGE("select1");
        k_select1<<<(B * S + 255) / 256, 256, 0, s>>>(2, rec, ncand, attG, attB, B, c, wl[WL_OSD]);
    } else {
        bp_fine(5, wl[WL_BP1], 0);
        STAGE("select1");
        k_select1<<<(B * S + 255) / 256, 256, 0, s>>>(3, rec, ncand, attG, attB, B, c, wl[WL_OSD]);
    }
    STAGE("osd");
    launch_osd(h, mt, ladder_grid(h, B * c.max_cands * 10), s, 0, llr0, saved, attB, rec, ncand, attO, ev, evc, h->d_trials, h->n_trials,
               osd_nflip(c.osd_single, c.osd_triple), c.osd_max_hd, sh, wl[WL_OSD], wl[WL_OSDNAN]);
    STAGE("select2");
    k_select2<<<(B * S + 255) / 256, 256, 0, s>>>(rec, ncand, attO, B, sh);
    if (h->ap.np) {
        // ipass 7 (ft8rx_set_ap_calls, kernels/ap_calls.hpp), after the whole reference ladder.  Scratch that is dead by now: the
        // candidate list in WL_BP0's items, the OSD list in WL_OSDNAN's, the attempt results in attO's slots.
        STAGE("ap_calls");
        ApCalls* apc = h->d_apc + chunk;
        if (h->ap_chunk_version[chunk] != h->ap_version) {       // this chunk's copy is stale: rewrite it behind the chunk's earlier work
            k_ap_stage<<<1, 64, 0, s>>>(apc, h->ap);
            h->ap_chunk_version[chunk] = h->ap_version;
        }
        launch_ap_calls(h, B, llr0, rec, ncand, attO, ev, evc, wl[WL_BP0].items, wl[WL_OSDNAN].items, h->d_apcount + 2 * chunk, apc, s);
    }
    if (sl.recall) {
        // ipass 8 (ft8rx_set_recall, kernels/recall.hpp), after the whole ladder: it reads the ladder's records (skip rule), and the
        // cycle spectrum it resamples still lies in this chunk's grid region -- only the next batch's k_spectrogram overwrites it
        STAGE("recall");
        ft8rx_recall_entry* ent = sl.d_rc_ent + F * FT8RX_RECALL_MAX;
        int32_t* rcnt = sl.d_rc_cnt + F;
        k_recall_stage<<<B, FT8RX_RECALL_MAX, 0, s>>>(h->d_rc_src + F * FT8RX_RECALL_MAX, h->d_rc_srccnt + F, ent, rcnt, sl.d_rc_rec + F * FT8RX_RECALL_MAX);
        const int base = h->rc_off[F], n = h->rc_off[F + B] - base;
        if (n > 0) {
            k_recall_trip<<<B, FT8RX_RECALL_MAX, 0, s>>>(ent, rcnt, h->d_rc_off + F, h->d_rc_trip);
            const size_t b = (size_t)base;
            launch_fine(h, c, false, n, s, spec, nullptr, nullptr, h->d_rc_llr + b * 174, h->d_rc_trip + 3 * b, h->d_rc_tout + 5 * b,
                        h->d_rc_tsd + b, h->d_rc_sgrid + b * 632, WorkList{nullptr, nullptr}, h->rc_td);     // rc_td: an entry beyond k_fine's h0 range
            k_recall_score<<<n, 64, 0, s>>>(h->d_rc_sgrid, h->d_rc_tout, h->d_rc_trip, h->d_rc_off + F, base, ent, rec, ncand, sh,
                                            h->rc_max_hd, h->rc_min_gap, sl.d_rc_rec + F * FT8RX_RECALL_MAX);
        }
    }
    if (sl.reports) {
        // measured reports (ft8rx_set_reports, kernels/report.hpp), after the last ladder step: the records are final, and the cycle
        // spectrum still lies in this chunk's grid region (as recall relies on)
        STAGE("report");
        launch_reports(h, B, spec, rec, ncand, h->d_rp_items + FS, h->d_rp_count + chunk, sl.d_rp + FS, s);
    }
    if (prof) hipEventRecord(h->pev[h->pnames.size()], s);
#undef STAGE
}

// A chunk's frames go through the WHOLE chain in cache-sized sub-batches, one after the other on the chunk's stream: a sub-batch's dB
// grid (1.47 MB per frame) is then still in L2 / the 256 MB MALL when k_sync, k_topk and k_grid_llr read it, and the four-step scratch
// and cycle spectrum that later overlay it are too when k_cyc_bc / k_fine read them -- a 4096-frame chunk's grid is 6 GB and every
// stage of it came from HBM (k_spectrogram 0.36 -> 0.42 ms per 256 frames, profiles/archive/r04_batch_sweep.txt).  Every workspace is indexed
// by frame and the chunk's work-list counters are re-zeroed by each chain's k_topk, so consecutive sub-batches on one stream need
// nothing but stream order.  Results do not depend on the partition (tests/test_gpu_parity.py: test_subbatch_partition_invariance).
static void enqueue_chunk(ft8rx_handle* h, const Frames& d_audio, int f0, int n, hipStream_t s, int slot, int chunk) {
    const int sub = (h->sub_frames > 0 && h->sub_frames < n) ? h->sub_frames : n;
    for (int o = 0; o < n; o += sub) enqueue_chain(h, d_audio, f0 + o, (o + sub <= n) ? sub : n - o, s, false, slot, chunk);
}

// Launch one batch: audio either resident on the device (Entry DEVICE) or copied from the host, in chunks (HOST_SYNC) or staged in
// the buffer of the batch's result slot (HOST_PIPELINED).  batch_plan.hpp decides how the batch is cut and ordered (one chain on the
// main stream, fork / join over the chunk streams, or free-running chunk streams) and says why.  Host audio of the synchronous entry
// is copied chunk by chunk in order on the dedicated copy stream (never queued behind kernels, so a pageable-memory copy blocks the
// host only for its own duration) and each chunk's chain waits for its copy's event.
// When the kernels are done the copy stream moves the slot's results into the page-locked host buffers (batch_finish).
// HOST_PIPELINED (ft8rx_enqueue_batch_host): the audio is staged in the buffer of this batch's result slot and its copy runs on
// its own stream, gated only by the previous user of that staging buffer (two batches ago), so it overlaps the kernels of
// the batch before.
using batchplan::BatchPlan;
using batchplan::Entry;

// Prologue: the result slot is taken (with both taken, the oldest unfetched batch is dropped), the per-batch settings are consumed,
// a host entry gets its staging buffer (*stage; a pipelined one waits for that buffer's last reader), and the chunk streams of a
// chunked batch are created on first use
static int batch_begin(ft8rx_handle* h, Entry e, int B, int slot, bool chunked, int sb, void** stage) {
    ResultSlot& sl = h->slots[slot];
    h->pnames.clear();
    // (first use of a staging buffer comes before anything of the handle changes: a failed one leaves it as it was)
    if (e != batchplan::DEVICE && need_staging(h, sb, false)) return -2;
    if (e == batchplan::HOST_PIPELINED && slot == 1 && need_staging(h, sb, true)) return -2;
    if (h->inflight == 2) { h->slot_fetch ^= 1; h->inflight = 1; }          // the oldest unfetched batch is dropped
    if (h->rc_armed && B != h->rc_frames) { set_err(h, "recall entries were set for %d frames, the batch has %d", h->rc_frames, B); return -1; }
    sl.recall = h->rc_armed;                     // ft8rx_set_recall: consumed by this batch
    h->rc_armed = false;
    sl.reports = h->reports;                     // ft8rx_set_reports: the setting this batch is enqueued with
    *stage = staging_of(h, sb, false);
    if (e == batchplan::HOST_PIPELINED) {
        *stage = staging_of(h, sb, slot != 0);
        HIPCHK(h, hipStreamWaitEvent(h->h2d_s, sl.ev_comp, 0));             // the kernels that last read this staging buffer are done
    }
    for (int i = 1; i < h->n_streams && chunked; i++) if (!h->sub[i - 1]) {
        if (!(h->sub[i - 1] = pool_sub(h->device, i - 1))) { set_err(h, "cannot create a chunk stream"); return -2; }
        HIPCHK(h, hipEventCreateWithFlags(&h->ev_join[i - 1], hipEventDisableTiming));
    }
    return 0;
}

// Submission: the plan's chunks, chunk k on stream k % n_streams (stream 0 = the main stream).  audio: on the device for Entry
// DEVICE, else on the host and copied to `stage` first, on `cs`.  The mode decides what precedes the chunks, what each chunk waits
// for, whether an empty chunk is skipped, and what follows them.
static int batch_submit(ft8rx_handle* h, const BatchPlan& plan, Entry e, int slot, const Frames& audio, void* stage) {
    ResultSlot& sl = h->slots[slot];
    const bool host = e != batchplan::DEVICE;
    const Frames d_audio = host ? Frames{stage, audio.sb} : audio; const char* host_audio = host ? (const char*)audio.p : nullptr;
    const int ns = h->n_streams, nc = plan.nc, B = plan.cb[nc];
    const bool free_run = plan.mode == batchplan::FREE_RUN, pipelined = e == batchplan::HOST_PIPELINED, sync_host = e == batchplan::HOST_SYNC;
    hipStream_t cs = pipelined ? h->h2d_s : h->copy_s;
    const size_t frame_bytes = audio.bytes(1);                 // host copies are sized by the sample bytes
    auto chunk_stream = [&](int k) { const int i = k % ns; return i == 0 ? h->stream : h->sub[i - 1]; };
    if (free_run) {
        for (int i = 0; i < ns; i++) for (int k = 0; k < 2; k++)
            if (!h->ev_cdone[k][i]) HIPCHK(h, hipEventCreateWithFlags(&h->ev_cdone[k][i], hipEventDisableTiming));
        if (h->need_barrier || h->part_B != B || h->part_n != nc) {
            // first batch of a run (or another partition): everything issued so far, on any stream of this handle, first
            if (h->free_running) HIPCHK(h, hipStreamWaitEvent(h->stream, h->slots[h->last_slot].ev_comp, 0));
            HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
            for (int i = 1; i < ns; i++) HIPCHK(h, hipStreamWaitEvent(h->sub[i - 1], h->ev_fork, 0));
            h->need_barrier = false; h->part_B = B; h->part_n = nc;
        }
    } else {
        { const int q = quiesce(h, true); if (q) return q; }
        HIPCHK(h, hipStreamWaitEvent(h->stream, sl.ev_done, 0));            // the slot's previous results have left the device
        if (plan.mode == batchplan::SINGLE) {
            if (host_audio) HIPCHK(h, hipMemcpyAsync(stage, host_audio, frame_bytes * B, hipMemcpyHostToDevice, h->stream));
            if (h->profiling) enqueue_chain(h, d_audio, 0, B, h->stream, true, slot, 0);      // per-stage events bracket whole-batch launches
            else enqueue_chunk(h, d_audio, 0, B, h->stream, slot, 0);
            return 0;
        }
        HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
        if (sync_host) HIPCHK(h, hipStreamWaitEvent(cs, h->ev_fork, 0));
        for (int i = 1; i < ns; i++) HIPCHK(h, hipStreamWaitEvent(h->sub[i - 1], h->ev_fork, 0));
    }
    if (pipelined) {
        // ONE copy for the whole batch and one event: it has the whole previous batch to hide behind, and a copy stream with
        // event markers BETWEEN its copies can stall on them (markers are queue packets: in a hardware queue shared with a
        // chunk stream they wait their turn behind that chunk's kernels -- the second of two chunk copies then started only
        // at the end of the previous batch, rocprofv3 trace in profiles/archive/r03_notes.md)
        HIPCHK(h, hipMemcpyAsync(stage, host_audio, frame_bytes * B, hipMemcpyHostToDevice, cs));
        HIPCHK(h, hipEventRecord(h->ev_chunk[0], cs));
        if (!free_run) for (int i = 0; i < ns; i++) HIPCHK(h, hipStreamWaitEvent(chunk_stream(i), h->ev_chunk[0], 0));
    }
    for (int k = 0; k < nc; k++) {
        const int f0 = plan.cb[k], n = plan.cb[k + 1] - f0;
        if (n <= 0 && !free_run) continue;
        hipStream_t s = chunk_stream(k);
        if (free_run) {
            HIPCHK(h, hipStreamWaitEvent(s, sl.ev_done, 0));                // the slot's previous results have left the device
            if (pipelined) HIPCHK(h, hipStreamWaitEvent(s, h->ev_chunk[0], 0));
        } else if (sync_host) {
            HIPCHK(h, hipMemcpyAsync((char*)stage + frame_bytes * f0, host_audio + frame_bytes * f0, frame_bytes * n, hipMemcpyHostToDevice, cs));
            HIPCHK(h, hipEventRecord(h->ev_chunk[k], cs));
            HIPCHK(h, hipStreamWaitEvent(s, h->ev_chunk[k], 0));
        }
        if (n > 0) enqueue_chunk(h, d_audio, f0, n, s, slot, k);
        if (free_run) {                                                     // only the result copy waits for every chunk
            HIPCHK(h, hipEventRecord(h->ev_cdone[slot][k], s));
            HIPCHK(h, hipStreamWaitEvent(h->copy_s, h->ev_cdone[slot][k], 0));
        }
    }
    if (free_run) h->free_running = true;
    else for (int i = 1; i < ns; i++) {
        HIPCHK(h, hipEventRecord(h->ev_join[i - 1], h->sub[i - 1]));
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_join[i - 1], 0));
    }
    return 0;
}

// Result tail: results -> page-locked host buffers on the copy stream (overlaps the next batch, which computes into the other slot).
// fin = the stream on which "all kernels of this batch are done" is known: the main stream after its joins, or -- free-running
// chunks -- the copy stream, which has just been made to wait for every chunk
static int batch_finish(ft8rx_handle* h, int slot, int B, hipStream_t fin) {
    ResultSlot& sl = h->slots[slot];
    const int mc = h->cfg.max_cands, sh = cand_shift(h->cfg);
    // The event log is [B][FT8RX_EVENT_CAP] x 24 B = 12 KB per frame of which a frame typically uses a tenth (config 1: ~40 events).
    // Small batches copy it whole (the latency case).  Large ones are packed: k_ev_compact writes the used entries -- and nothing
    // else -- into page-locked host memory: ~8 MB instead of 100 MB per 8192-frame shard on the host link.
    // (A copy-engine transfer of the packed run is not an option: an asynchronous device-to-host copy of a few hundred KB takes the
    // runtime's shader-copy path, which queued behind the next batch's kernels and cost 0.5 ms per 256-frame step.)
    const bool pack_events = sl.d_evpacked && (size_t)B * FT8RX_EVENT_CAP * sizeof(ft8rx_event) > EV_EAGER_BYTES;
    if (pack_events) {
        k_ev_scan<<<1, 1024, 0, fin>>>(sl.evcount, B, sl.d_evoffs);
        k_ev_compact<<<B, 64, 0, fin>>>(sl.ev, sl.evcount, sl.d_evoffs, sl.d_evpacked);
    }
    sl.packed = sl.pk_buf != nullptr;
    if (sl.packed) {                                         // packed results for a gather: header | frame table | kept records | used events
        if (sl.pk_fence) { HIPCHK(h, hipStreamWaitEvent(fin, sl.pk_fence, 0)); sl.pk_fence = nullptr; }      // the consumer's asynchronous read of this buffer
        k_pack_count<<<B, 256, 0, fin>>>(sl.rec, sl.ncand, sl.ev, sl.evcount, h->d_pkneed, h->d_pknrec, sh);
        k_pack_scan<<<1, 1024, 0, fin>>>(h->d_pknrec, sl.ncand, sl.evcount, B, mc, (unsigned long long)h->pk_cap, sl.pk_buf, sl.d_pkhdr);
        k_pack_write<<<B, 256, 0, fin>>>(sl.rec, sl.ev, h->d_pkneed, B, sl.pk_buf, sh);
    }
    HIPCHK(h, hipEventRecord(sl.ev_comp, fin));
    if (fin != h->copy_s) HIPCHK(h, hipStreamWaitEvent(h->copy_s, sl.ev_comp, 0));
    HIPCHK(h, hipMemcpyAsync(sl.h_cnt, sl.ncand, sizeof(int32_t) * B, hipMemcpyDeviceToHost, h->copy_s));
    HIPCHK(h, hipMemcpy2DAsync(sl.h_rec, sizeof(ft8rx_record) * mc, sl.rec, sizeof(ft8rx_record) << sh, sizeof(ft8rx_record) * mc, B, hipMemcpyDeviceToHost, h->copy_s));
    HIPCHK(h, hipMemcpyAsync(sl.h_evc, sl.evcount, sizeof(int32_t) * B, hipMemcpyDeviceToHost, h->copy_s));
    sl.evpending = pack_events;
    if (!pack_events) HIPCHK(h, hipMemcpyAsync(sl.h_ev, sl.ev, sizeof(ft8rx_event) * (size_t)B * FT8RX_EVENT_CAP, hipMemcpyDeviceToHost, h->copy_s));
    if (sl.recall) {
        HIPCHK(h, hipMemcpyAsync(sl.h_rc_cnt, sl.d_rc_cnt, sizeof(int32_t) * B, hipMemcpyDeviceToHost, h->copy_s));
        HIPCHK(h, hipMemcpyAsync(sl.h_rc_rec, sl.d_rc_rec, sizeof(ft8rx_record) * FT8RX_RECALL_MAX * (size_t)B, hipMemcpyDeviceToHost, h->copy_s));
    }
    if (sl.reports)
        HIPCHK(h, hipMemcpy2DAsync(sl.h_rp, sizeof(ft8rx_report) * mc, sl.d_rp, sizeof(ft8rx_report) << sh, sizeof(ft8rx_report) * mc, B, hipMemcpyDeviceToHost, h->copy_s));
    HIPCHK(h, hipEventRecord(sl.ev_done, h->copy_s));
    sl.B = B; h->last_slot = slot; h->slot_enq ^= 1; h->inflight++;
    return 0;
}

// audio: on the device for Entry DEVICE, else on the host
static int launch_batch(ft8rx_handle* h, Entry e, const Frames& audio, int B) {
    HIPCHK(h, hipSetDevice(h->device));
    const BatchPlan plan = batchplan::plan_batch(B, h->n_streams, h->profiling, e);
    const int slot = h->slot_enq;
    void* stage = nullptr;
    if (const int rc = batch_begin(h, e, B, slot, plan.mode != batchplan::SINGLE, audio.sb, &stage)) return rc;
    if (const int rc = batch_submit(h, plan, e, slot, audio, stage)) return rc;
    HIPCHK(h, hipGetLastError());
    return batch_finish(h, slot, B, plan.mode == batchplan::FREE_RUN ? h->copy_s : h->stream);
}

// Large batches: the packed event log (k_ev_compact, written by the GPU into page-locked memory) -> the [frame][FT8RX_EVENT_CAP] rows
// of h_ev that the fetch functions hand out.  The per-frame counts have arrived, so the host knows each frame's offset in the
// packed run (the same prefix sum k_ev_scan made).  Rows beyond a frame's count are not written.
static void fetch_events(ResultSlot& sl) {
    if (!sl.evpending) return;
    size_t off = 0;
    for (int f = 0; f < sl.B; f++) {
        int c = sl.h_evc[f]; c = c > FT8RX_EVENT_CAP ? FT8RX_EVENT_CAP : (c < 0 ? 0 : c);
        if (c) memcpy(sl.h_ev + (size_t)f * FT8RX_EVENT_CAP, sl.h_evpacked + off, sizeof(ft8rx_event) * (size_t)c);
        off += (size_t)c;
    }
    sl.evpending = false;
}

int ft8rx_enqueue_batch(ft8rx_handle* h, const int16_t* d_audio, int B) {
    if (!h || !d_audio) return -1;
    if (B < 1 || B > h->max_frames) { set_err(h, "ft8rx_enqueue_batch: n_frames %d outside [1, %d]", B, h->max_frames); return -1; }
    return launch_batch(h, batchplan::DEVICE, Frames{d_audio, 2}, B);
}

int ft8rx_enqueue_batch_host(ft8rx_handle* h, const int16_t* audio, int B) {
    if (!h || !audio) return -1;
    if (B < 1 || B > h->max_frames) { set_err(h, "ft8rx_enqueue_batch_host: n_frames %d outside [1, %d]", B, h->max_frames); return -1; }
    return launch_batch(h, batchplan::HOST_PIPELINED, Frames{audio, 2}, B);
}

// float32 frames: the same plan, chunks, slots and streams; the kernels load sample pairs as 8-byte words
static bool f32_aligned(ft8rx_handle* h, const char* who, const float* d_audio) {
    if (((uintptr_t)d_audio % 8) == 0) return true;
    set_err(h, "%s: d_audio is not aligned to 8 bytes (a pair of float32 samples)", who);
    return false;
}
int ft8rx_enqueue_batch_f32(ft8rx_handle* h, const float* d_audio, int B) {
    if (!h || !d_audio) return -1;
    if (B < 1 || B > h->max_frames) { set_err(h, "ft8rx_enqueue_batch_f32: n_frames %d outside [1, %d]", B, h->max_frames); return -1; }
    if (!f32_aligned(h, "ft8rx_enqueue_batch_f32", d_audio)) return -1;
    return launch_batch(h, batchplan::DEVICE, Frames{d_audio, 4}, B);
}

int ft8rx_enqueue_batch_host_f32(ft8rx_handle* h, const float* audio, int B) {
    if (!h || !audio) return -1;
    if (B < 1 || B > h->max_frames) { set_err(h, "ft8rx_enqueue_batch_host_f32: n_frames %d outside [1, %d]", B, h->max_frames); return -1; }
    return launch_batch(h, batchplan::HOST_PIPELINED, Frames{audio, 4}, B);
}

int ft8rx_set_streams(ft8rx_handle* h, int n) { if (!h || n < 1 || n > batchplan::MAX_STREAMS) return -1; h->n_streams = n; return 0; }
int ft8rx_set_subbatch(ft8rx_handle* h, int frames) { if (!h || frames < 0) return -1; h->sub_frames = frames; return 0; }
int ft8rx_set_ladder_mode(ft8rx_handle* h, int mode) { if (!h || mode < 0 || mode > 1) return -1; h->ladder_mode = mode; return 0; }

int ft8rx_set_ladder_grid(ft8rx_handle* h, int cap) {
    if (!h) return -1;
    if (cap < 0 || cap > LADDER_GRID_CAP) { set_err(h, "ft8rx_set_ladder_grid: cap %d outside [0, %d] (0 = the default, %d)", cap, LADDER_GRID_CAP, LADDER_GRID_CAP); return -1; }
    ENTER(h);                                   // batches in flight were launched under the previous cap
    h->ladder_cap = cap ? cap : LADDER_GRID_CAP;
    return 0;
}

int ft8rx_set_weak(ft8rx_handle* h, int32_t on, float sync_min, int32_t osd_max_hd) {
    if (!h) return -1;
    if (on) {
        if (!(sync_min > 0.0f) || !(sync_min < INFINITY)) { set_err(h, "ft8rx_set_weak: sync_min %g must be a positive score", (double)sync_min); return -1; }
        if (osd_max_hd < 1 || osd_max_hd > 174) { set_err(h, "ft8rx_set_weak: osd_max_hd %d outside [1, 174]", osd_max_hd); return -1; }
        if (refuse_conflict(h, "ft8rx_set_weak", optins::WEAK)) return -1;
        h->weak_sync_min = sync_min; h->weak_osd_max_hd = osd_max_hd;
    }
    h->weak = on != 0;                          // batches in flight keep the setting they were enqueued with (enqueue_chain reads it)
    return 0;
}

int ft8rx_set_msg_types(ft8rx_handle* h, int32_t mask) {
    if (!h) return -1;
    if (mask < 0 || mask > FT8RX_MT_ALL) { set_err(h, "ft8rx_set_msg_types: mask %d outside [0, %d]", mask, FT8RX_MT_ALL); return -1; }
    if (mask && refuse_conflict(h, "ft8rx_set_msg_types", optins::MSG_TYPES)) return -1;
    h->msg_types = mask;                        // batches in flight keep the setting they were enqueued with (enqueue_chain reads it)
    return 0;
}

// ipass-7 patterns of (my, dx) (kernels/ap_patterns.hpp); NULL / "" = unset.  -> 0, or -1 with the reason in err
static int build_ap_patterns(const char* my, const char* dx, ApCalls* a, std::string* err) {
    const bool hm = my && *my, hd = dx && *dx;
    const long cm = hm ? hostmsg::pack_c28_std(my) : 0, cd = hd ? hostmsg::pack_c28_std(dx) : 0;
    if (cm < 0) { *err = std::string("my_call '") + my + "' is not a standard callsign"; return -1; }
    if (cd < 0) { *err = std::string("dx_call '") + dx + "' is not a standard callsign"; return -1; }
    const int32_t max_hd = a->max_hd;
    memset(a, 0, sizeof(*a)); a->max_hd = max_hd;
    // 77-bit i3 = 1 word: c28 r1 c28 r1 R1 g15 i3; position i (LLR order) = word bit 76 - i
    auto word = [](long c1, long c2, unsigned g15) { return ((unsigned __int128)c1 << 49) | ((unsigned __int128)c2 << 20) | ((unsigned __int128)g15 << 3) | 1u; };
    const unsigned G_RRR = 32402, G_73 = 32404, G_RR73 = 32403;
    for (int p = 5; p <= 10; p++) {
        const bool on = p == 5 ? hm : p == 7 ? hd : (hm && hd);
        if (!on) continue;
        const int k = p - FT8RX_AP_FIRST;
        const unsigned __int128 w = word(p == 7 ? 2 : cm, p == 5 ? 0 : cd, p == 8 ? G_RRR : p == 9 ? G_73 : G_RR73);
        const uint64_t lo = (uint64_t)w, hi = (uint64_t)(w >> 64);
        if (p >= 8) {
            hostmsg::encode_cw174(lo, hi, a->val[k]);
            a->msk[k][0] = a->msk[k][1] = ~0ull; a->msk[k][2] = (1ull << 46) - 1;
            a->lo[k] = lo; a->hi[k] = hi;
            hostmsg::Hashes H; std::string f[3];
            if (!hostmsg::unpack_ext(lo, hi, 0, H, f)) { *err = "the words of my_call / dx_call do not unpack as a standard message"; return -1; }
        } else {
            const int nk = p == 5 ? 29 : 58;                                // known call fields: positions 0 .. nk - 1, and i3 (74 .. 76)
            for (int i = 0; i < 77; i++) {
                if (!(i < nk || i >= 74)) continue;
                const unsigned b = (unsigned)((w >> (76 - i)) & 1u);
                a->msk[k][i >> 6] |= 1ull << (i & 63);
                if (b) a->val[k][i >> 6] |= 1ull << (i & 63);
            }
        }
        a->pat[a->np++] = p;
    }
    return 0;
}

int ft8rx_set_ap_calls(ft8rx_handle* h, const char* my_call, const char* dx_call) {
    if (!h) return -1;
    ApCalls a = h->ap;
    std::string err;
    if (build_ap_patterns(my_call, dx_call, &a, &err)) { set_err(h, "ft8rx_set_ap_calls: %s", err.c_str()); return -1; }
    if (a.np && refuse_conflict(h, "ft8rx_set_ap_calls", optins::AP_CALLS)) return -1;
    h->ap = a; h->ap_version++;                 // batches in flight keep the setting they were enqueued with (enqueue_chain)
    return 0;
}

int ft8rx_set_ap_max_hd(ft8rx_handle* h, int32_t max_hd) {
    if (!h) return -1;
    if (max_hd < 1 || max_hd > 174) { set_err(h, "ft8rx_set_ap_max_hd: %d outside [1, 174]", max_hd); return -1; }
    h->ap.max_hd = max_hd; h->ap_version++;
    return 0;
}

int ft8rx_ap_patterns(const char* my_call, const char* dx_call, uint8_t* bits_out, uint8_t* mask_out) {
    ApCalls a = ap_calls_off();
    std::string err;
    if (build_ap_patterns(my_call, dx_call, &a, &err)) { g_create_err = "ft8rx_ap_patterns: " + err; return -1; }
    for (int k = 0; k < FT8RX_AP_N; k++) for (int i = 0; i < 174; i++) {
        if (bits_out) bits_out[k * 174 + i] = (uint8_t)((a.val[k][i >> 6] >> (i & 63)) & 1ull);
        if (mask_out) mask_out[k * 174 + i] = (uint8_t)((a.msk[k][i >> 6] >> (i & 63)) & 1ull);
    }
    return 0;
}

// recall (kernels/recall.hpp): the kind of an entry's word -- RC_CALL "A B X", RC_TOKEN "CQ / QRZ / DE B X", RC_SKIP anything else
static int recall_kind(uint64_t lo, uint64_t hi) {
    const unsigned i3 = (unsigned)(lo & 7u);
    if (i3 != 1 && i3 != 2) return RC_SKIP;
    const uint64_t ca = ((lo >> 49) | (hi << 15)) & 0xFFFFFFFull, cb = (lo >> 20) & 0xFFFFFFFull;
    const uint64_t STD = 2063592ull + 4194304ull;                           // NTOKENS + MAX22: the first standard call
    if (cb < STD || !(ca < 3 || ca >= STD)) return RC_SKIP;
    hostmsg::Hashes H; std::string f[3];
    if (!hostmsg::unpack_ext(lo, hi & 0x1FFFull, 0, H, f)) return RC_SKIP;
    for (int k = 0; k < 3; k++) if (f[k].find('<') != std::string::npos) return RC_SKIP;
    return ca < 3 ? RC_TOKEN : RC_CALL;
}

int ft8rx_recall_hypotheses(const ft8rx_recall_entry* entry, uint64_t* words_lo, uint64_t* words_hi) {
    if (!entry) return -1;
    const uint64_t lo = entry->msg_lo, hi = entry->msg_hi & 0x1FFFull;
    const int kind = recall_kind(lo, hi);
    if (kind == RC_SKIP) return 0;
    int n = 0;
    for (int k = 0; k < 126; k++) {                 // the device's list (recall_word), the repeat's duplicate dropped
        uint64_t w; unsigned g15 = 0, r = 0;
        if (k == 0) w = lo;
        else if (kind != RC_CALL) break;
        else {
            if (k <= 3) g15 = 32401u + (unsigned)k;
            else if (k < 65) g15 = (unsigned)(32435 + (k - 4) - 30);
            else { g15 = (unsigned)(32435 + (k - 65) - 30); r = 1; }
            w = (lo & ~(0xFFFFull << 3)) | ((uint64_t)g15 << 3) | ((uint64_t)r << 18);
            if (w == lo) continue;
        }
        if (words_lo) words_lo[n] = w;
        if (words_hi) words_hi[n] = hi;
        n++;
    }
    return n;
}

static int recall_alloc(ft8rx_handle* h) {
    if (ws_ready(h, WS_RECALL)) return 0;
    const size_t B = (size_t)h->max_frames, N = B * FT8RX_RECALL_MAX;
    FirstUse F(h, WS_RECALL);
    F.dev(&h->d_rc_src, N); F.dev(&h->d_rc_srccnt, B); F.dev(&h->d_rc_off, B + 1);
    F.dev(&h->d_rc_trip, N * 3); F.dev(&h->d_rc_tout, N * 5); F.dev(&h->d_rc_tsd, N);
    F.dev(&h->d_rc_sgrid, N * 632); F.dev(&h->d_rc_llr, N * 174);
    for (ResultSlot& sl : h->slots) {
        F.dev(&sl.d_rc_ent, N); F.dev(&sl.d_rc_cnt, B); F.dev(&sl.d_rc_rec, N);
        F.host(&sl.h_rc_rec, N); F.host(&sl.h_rc_cnt, B);
    }
    return F.done();
}

int ft8rx_set_recall(ft8rx_handle* h, const ft8rx_recall_entry* entries, const int32_t* counts, int n_frames) {
    if (!h) return -1;
    ENTER(h);                                   // batches in flight were enqueued under the previous setting
    if (!entries || n_frames == 0) { h->rc_armed = false; return 0; }
    if (!counts || n_frames < 1 || n_frames > h->max_frames) { set_err(h, "ft8rx_set_recall: n_frames %d outside [1, %d]", n_frames, h->max_frames); return -1; }
    if (refuse_conflict(h, "ft8rx_set_recall", optins::RECALL)) return -1;
    const ft8rx_config& c = h->cfg;
    std::vector<ft8rx_recall_entry> st((size_t)n_frames * FT8RX_RECALL_MAX);
    std::vector<int32_t> cnt(n_frames), off(n_frames + 1, 0);
    bool td = false;
    for (int f = 0; f < n_frames; f++) {
        if (counts[f] < 0 || counts[f] > FT8RX_RECALL_MAX) { set_err(h, "ft8rx_set_recall: counts[%d] = %d outside [0, %d]", f, counts[f], FT8RX_RECALL_MAX); return -1; }
        cnt[f] = counts[f]; off[f + 1] = off[f] + counts[f];
        for (int e = 0; e < counts[f]; e++) {
            ft8rx_recall_entry E = entries[(size_t)f * FT8RX_RECALL_MAX + e];
            if (E.f0_idx < c.f0_lo || E.f0_idx >= c.f0_hi || E.h0_idx < c.h0_lo || E.h0_idx >= c.h0_hi) {
                set_err(h, "ft8rx_set_recall: entry %d of frame %d at (f0_idx %d, h0_idx %d) lies outside the search range", e, f, E.f0_idx, E.h0_idx); return -1; }
            E.pad = (uint16_t)recall_kind(E.msg_lo, E.msg_hi);
            td |= E.h0_idx < FT8RX_MIN_H0_FD || E.h0_idx > FT8RX_MAX_H0_FD;
            st[(size_t)f * FT8RX_RECALL_MAX + e] = E;
        }
    }
    if (recall_alloc(h)) return -2;
    HIPCHK(h, hipMemcpy(h->d_rc_src, st.data(), sizeof(ft8rx_recall_entry) * st.size(), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_rc_srccnt, cnt.data(), sizeof(int32_t) * cnt.size(), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_rc_off, off.data(), sizeof(int32_t) * off.size(), hipMemcpyHostToDevice));
    h->rc_off = off; h->rc_frames = n_frames; h->rc_td = td; h->rc_armed = true;
    return 0;
}

int ft8rx_fetch_recall(ft8rx_handle* h, int n_frames, ft8rx_record* records, int32_t* counts) {
    if (!h) return -1;
    const int slot = h->fetched_slot;
    if (slot < 0) { set_err(h, "ft8rx_fetch_recall: no batch has been fetched"); return -1; }
    const ResultSlot& sl = h->slots[slot];
    if (n_frames < 1 || n_frames > sl.B) { set_err(h, "ft8rx_fetch_recall: %d frames requested, the batch had %d", n_frames, sl.B); return -1; }
    HIPCHK(h, hipEventSynchronize(sl.ev_done));
    if (!sl.recall) {
        if (counts) memset(counts, 0, sizeof(int32_t) * n_frames);
        if (records) memset(records, 0, sizeof(ft8rx_record) * FT8RX_RECALL_MAX * (size_t)n_frames);
        return 0;
    }
    if (counts) memcpy(counts, sl.h_rc_cnt, sizeof(int32_t) * n_frames);
    if (records) memcpy(records, sl.h_rc_rec, sizeof(ft8rx_record) * FT8RX_RECALL_MAX * (size_t)n_frames);
    return 0;
}

int ft8rx_set_reports(ft8rx_handle* h, int32_t on) {
    if (!h) return -1;
    ENTER(h);                                   // batches in flight were enqueued under the previous setting
    if (!on) { h->reports = false; return 0; }
    if (refuse_conflict(h, "ft8rx_set_reports", optins::REPORTS)) return -1;
    if (!ws_ready(h, WS_REPORTS)) {
        const size_t B = (size_t)h->max_frames, N = B << cand_shift(h->cfg);
        FirstUse F(h, WS_REPORTS);
        F.dev(&h->d_rp_items, N); F.dev(&h->d_rp_count, (size_t)batchplan::MAX_CHUNKS);
        for (ResultSlot& sl : h->slots) { F.dev(&sl.d_rp, N); F.host(&sl.h_rp, B * h->cfg.max_cands); }
        if (F.done()) return -2;
    }
    h->reports = true;
    return 0;
}

int ft8rx_fetch_reports(ft8rx_handle* h, int n_frames, ft8rx_report* reports) {
    if (!h || !reports) return -1;
    const int slot = h->fetched_slot;
    if (slot < 0) { set_err(h, "ft8rx_fetch_reports: no batch has been fetched"); return -1; }
    const ResultSlot& sl = h->slots[slot];
    if (n_frames < 1 || n_frames > sl.B) { set_err(h, "ft8rx_fetch_reports: %d frames requested, the batch had %d", n_frames, sl.B); return -1; }
    HIPCHK(h, hipEventSynchronize(sl.ev_done));
    const size_t bytes = sizeof(ft8rx_report) * (size_t)n_frames * h->cfg.max_cands;
    if (!sl.reports) memset(reports, 0, bytes);
    else memcpy(reports, sl.h_rp, bytes);
    return 0;
}

int ft8rx_set_recall_gates(ft8rx_handle* h, int32_t max_hd, int32_t min_gap) {
    if (!h) return -1;
    if (max_hd < 1 || max_hd > 174 || min_gap < 0 || min_gap > 174) { set_err(h, "ft8rx_set_recall_gates: max_hd %d / min_gap %d outside [1, 174] / [0, 174]", max_hd, min_gap); return -1; }
    h->rc_max_hd = max_hd; h->rc_min_gap = min_gap;
    return 0;
}

// ---------------------------------------------------------------------------- down-converter
// Kaiser-windowed sinc, odd length from the Kaiser estimate, cutoff half way between pass and stop edge, DC gain 1 (dc_gain: the rational resampler's L); designed in
// double, rounded once
static double ddc_bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 200; k++) { term *= (x / (2.0 * k)) * (x / (2.0 * k)); sum += term; if (term < 1e-20 * sum) break; }
    return sum;
}
static std::vector<float> ddc_design(double f_pass, double f_stop, double A, double fs, double dc_gain = 1.0) {
    int N = (int)ceil((A - 7.95) / (2.285 * 2.0 * M_PI * (f_stop - f_pass) / fs)) + 1;
    if (N % 2 == 0) N++;
    const double beta = 0.1102 * (A - 8.7), fc = (f_pass + f_stop) / (2.0 * fs), c = (N - 1) / 2.0;
    std::vector<double> h(N);
    double sum = 0.0;
    for (int n = 0; n < N; n++) {
        const double x = n - c, r = x / c;
        const double sinc = x == 0.0 ? 2.0 * fc : sin(2.0 * M_PI * fc * x) / (M_PI * x);
        h[n] = sinc * ddc_bessel_i0(beta * sqrt(1.0 - r * r)) / ddc_bessel_i0(beta);
        sum += h[n];
    }
    std::vector<float> out(N);
    for (int n = 0; n < N; n++) out[n] = (float)(dc_gain * (h[n] / sum));
    return out;
}
struct DdcTaps { std::vector<float> h1[3], h2[2]; };      // h1: D = 4, 8, 16; h2: at 24 kHz, at 12 kHz (D = 1)
static const DdcTaps& ddc_taps() {
    static const DdcTaps T = [] {
        DdcTaps t;
        for (int i = 0; i < 3; i++) t.h1[i] = ddc_design(3200.0, 20800.0, 85.0, 48000.0 * (1 << i));
        t.h2[0] = ddc_design(2800.0, 3200.0, 75.0, 24000.0);
        t.h2[1] = ddc_design(2800.0, 3200.0, 75.0, 12000.0);
        return t;
    }();
    return T;
}
static int ddc_decimation(int32_t rate_hz) {               // D, or 0 for a rate the build does not take
    for (int D = 1; D <= 16; D *= 2) if (rate_hz == 12000 * D) return D;
    return 0;
}
static const std::vector<float>* ddc_stage_taps(int D, int stage) {      // nullptr: the rate has no such stage
    const DdcTaps& T = ddc_taps();
    if (stage == 2) return &T.h2[D == 1];
    return D >= 4 ? &T.h1[D == 4 ? 0 : D == 8 ? 1 : 2] : nullptr;
}

int ft8rx_ddc_taps(int32_t rate_hz, int stage, float* taps, int cap) {
    const int D = ddc_decimation(rate_hz);
    if (!D || (stage != 1 && stage != 2)) return -1;
    const std::vector<float>* t = ddc_stage_taps(D, stage);
    if (!t) return 0;
    for (int i = 0; taps && i < cap && i < (int)t->size(); i++) taps[i] = (*t)[i];
    return (int)t->size();
}

static int ddc_workspaces(ft8rx_handle* h) {
    if (ws_ready(h, WS_DDC)) return 0;
    const DdcTaps& T = ddc_taps();
    static_assert(sizeof(c_ddc_h1) == sizeof(float) * 3 * 64 && sizeof(c_ddc_h2) == sizeof(float) * 2 * 288, "tap tables");
    std::vector<float> a(3 * 64, 0.0f), b(2 * 288, 0.0f);
    for (int i = 0; i < 3; i++) { if (T.h1[i].size() > 64) return -2; memcpy(&a[i * 64], T.h1[i].data(), sizeof(float) * T.h1[i].size()); }
    for (int i = 0; i < 2; i++) { if (T.h2[i].size() > 288) return -2; memcpy(&b[i * 288], T.h2[i].data(), sizeof(float) * T.h2[i].size()); }
    if (T.h1[0].size() != 17 || T.h1[1].size() != 31 || T.h1[2].size() != 61 || T.h2[0].size() != 283 || T.h2[1].size() != 143) {
        set_err(h, "ft8rx_ddc: the designed filters do not have the lengths the kernels were compiled for"); return -2;
    }
    FirstUse F(h, WS_DDC);
    F.dev(&h->d_ddc_outs, (size_t)h->max_frames);
    F.host(&h->h_ddc_outs, (size_t)h->max_frames);
    FIRST_HIP(F, hipMemcpyToSymbol(HIP_SYMBOL(c_ddc_h1), a.data(), sizeof(float) * a.size()));
    FIRST_HIP(F, hipMemcpyToSymbol(HIP_SYMBOL(c_ddc_h2), b.data(), sizeof(float) * b.size()));
    return F.done();
}

// the argument checks both entries share (everything but the input pointer) -> D, or -1 with the error text
static int ddc_check(ft8rx_handle* h, const char* who, int kind, int32_t rate_hz, int n_streams, uint64_t stream_stride, uint64_t n_samples,
                     int n_out, const int32_t* src, const double* f_dial_hz, float gain) {
    if (!sf_kind_in(SF_KINDS_DDC, kind)) { set_err(h, "%s: kind %d is not one of FT8RX_DDC_REAL_I16 .. FT8RX_DDC_IQ_F32", who, kind); return -1; }
    const int D = ddc_decimation(rate_hz);
    if (!D) { set_err(h, "%s: rate_hz %d is not 12000 x 1, 2, 4, 8 or 16", who, (int)rate_hz); return -1; }
    if (kind == FT8RX_DDC_REAL_I16 && D == 1) { set_err(h, "%s: kind real int16 at rate_hz 12000 is a frame already", who); return -1; }
    if (n_streams < 1) { set_err(h, "%s: n_streams %d < 1", who, n_streams); return -1; }
    if (n_out < 1 || n_out > h->max_frames) { set_err(h, "%s: n_out %d outside [1, %d] (max_frames)", who, n_out, h->max_frames); return -1; }
    if (n_samples > (uint64_t)FT8RX_NSAMP * D) { set_err(h, "%s: n_samples %llu > %d (15 s at rate_hz)", who, (unsigned long long)n_samples, FT8RX_NSAMP * D); return -1; }
    if (stream_stride < n_samples || stream_stride > ((uint64_t)1 << 40)) { set_err(h, "%s: stream_stride %llu does not hold n_samples %llu", who, (unsigned long long)stream_stride, (unsigned long long)n_samples); return -1; }
    if (!src || !f_dial_hz) { set_err(h, "%s: src / f_dial_hz is NULL", who); return -1; }
    for (int j = 0; j < n_out; j++) {
        if (src[j] < 0 || src[j] >= n_streams) { set_err(h, "%s: src[%d] = %d outside [0, %d) (n_streams)", who, j, (int)src[j], n_streams); return -1; }
        if (!(f_dial_hz[j] >= -0.5 * rate_hz && f_dial_hz[j] < 0.5 * rate_hz)) { set_err(h, "%s: f_dial_hz[%d] = %g outside [-rate_hz / 2, rate_hz / 2)", who, j, f_dial_hz[j]); return -1; }
    }
    if (!(fabsf(gain) <= 3.0e38f)) { set_err(h, "%s: gain is not finite", who); return -1; }
    return D;
}

// the channel table of n_out outputs: frequency words, sorted by stream (so that outputs of one stream run next to each other and share
// its loads in L2); f_mixed_hz: optional, the dials really mixed
static void ddc_table(DdcOut* outs, int32_t rate_hz, int n_out, const int32_t* src, const double* f_dial_hz, double* f_mixed_hz) {
    for (int j = 0; j < n_out; j++) {
        const double r = nearbyint((f_dial_hz[j] + 3000.0) / (double)rate_hz * 4294967296.0);
        const uint32_t w = (uint32_t)((long long)r & 0xffffffffLL);
        outs[j] = DdcOut{src[j], j, w, 0u};
        if (f_mixed_hz) {
            double f = (double)w * (double)rate_hz / 4294967296.0 - 3000.0;
            if (f >= 0.5 * rate_hz) f -= (double)rate_hz;
            f_mixed_hz[j] = f;
        }
    }
    std::stable_sort(outs, outs + n_out, [](const DdcOut& a, const DdcOut& b) { return a.src < b.src; });
}

// the launch: channel table (sorted by stream, so that outputs of one stream run next to each other and share its loads in L2) -> device,
// one kernel on the main stream
static int ddc_launch(ft8rx_handle* h, int D, const void* d_in, int fmt, int32_t rate_hz, uint64_t stream_stride, uint64_t n_samples, int n_out,
                      const int32_t* src, const double* f_dial_hz, float gain, int16_t* d_audio, float* d_audio_f32, double* f_mixed_hz) {
    if (!h->ddc_ev) HIPCHK(h, hipEventCreateWithFlags(&h->ddc_ev, hipEventDisableTiming));
    else HIPCHK(h, hipEventSynchronize(h->ddc_ev));      // the previous call's table has left the page-locked buffer (long ago, as a rule)
    DdcOut* outs = h->h_ddc_outs;
    ddc_table(outs, rate_hz, n_out, src, f_dial_hz, f_mixed_hz);
    HIPCHK(h, hipMemcpyAsync(h->d_ddc_outs, outs, sizeof(DdcOut) * (size_t)n_out, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(h->ddc_ev, h->stream));
    const float scale = gain * sf_real_gain(fmt);
    const unsigned grid = (unsigned)n_out * DDC_TILES;
    const unsigned long long ss = stream_stride; const int ns = (int)n_samples;
#define DDC_GO(DD) k_ddc<DD><<<grid, DDC_NT, 0, h->stream>>>(d_in, fmt, ss, ns, h->d_ddc_outs, scale, d_audio, d_audio_f32)
    switch (D) { case 1: DDC_GO(1); break; case 2: DDC_GO(2); break; case 4: DDC_GO(4); break; case 8: DDC_GO(8); break; default: DDC_GO(16); }
#undef DDC_GO
    HIPCHK(h, hipGetLastError());
    return 0;
}

int ft8rx_ddc(ft8rx_handle* h, const void* d_in, int kind, int32_t rate_hz, int n_streams, uint64_t stream_stride, uint64_t n_samples,
              int n_out, const int32_t* src, const double* f_dial_hz, float gain, int16_t* d_audio, float* d_audio_f32, double* f_mixed_hz) {
    if (!h) return -1;
    const int D = ddc_check(h, "ft8rx_ddc", kind, rate_hz, n_streams, stream_stride, n_samples, n_out, src, f_dial_hz, gain);
    if (D < 0) return -1;
    const int fmt = sample_fmt(kind);
    if (!d_in || ((uintptr_t)d_in % sf_sample_bytes(fmt)) != 0) { set_err(h, "ft8rx_ddc: d_in is NULL or not aligned to a sample"); return -1; }
    ENTER(h);
    if (ddc_workspaces(h)) return -2;
    if (!d_audio) { if (need_staging(h)) return -2; d_audio = h->d_audio; }
    return ddc_launch(h, D, d_in, fmt, rate_hz, stream_stride, n_samples, n_out, src, f_dial_hz, gain, d_audio, d_audio_f32, f_mixed_hz);
}

// hand one allocation of the handle back (ft8rx_ddc_stream_close; everything else lives until ft8rx_destroy)
static void release_dev(ft8rx_handle* h, void* p) {
    if (!p) return;
    for (size_t i = 0; i < h->allocs.size(); i++) if (h->allocs[i] == p) { h->allocs.erase(h->allocs.begin() + i); break; }
    hipFree(p);
}
static void release_host(ft8rx_handle* h, void* p) {
    if (!p) return;
    for (size_t i = 0; i < h->pinned.size(); i++) if (h->pinned[i] == p) { h->pinned.erase(h->pinned.begin() + i); break; }
    hipHostFree(p);
}
// a handle-owned device buffer that only grows: first use, or a larger call (nothing of the handle reads the old one any more)
static int grow_dev(ft8rx_handle* h, const char* who, void** p, size_t* cap, size_t bytes) {
    if (*cap >= bytes && *p) return 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes ? bytes : 256);
    if (e != hipSuccess) { set_err(h, "%s: hipMalloc(%zu bytes) failed: %s", who, bytes, hipGetErrorString(e)); return -2; }
    release_dev(h, *p);
    h->allocs.push_back(q); *p = q; *cap = bytes ? bytes : 256;
    return 0;
}

int ft8rx_ddc_host(ft8rx_handle* h, const void* in, int kind, int32_t rate_hz, int n_streams, uint64_t stream_stride, uint64_t n_samples,
                   int n_out, const int32_t* src, const double* f_dial_hz, float gain, double* f_mixed_hz) {
    if (!h) return -1;
    const int D = ddc_check(h, "ft8rx_ddc_host", kind, rate_hz, n_streams, stream_stride, n_samples, n_out, src, f_dial_hz, gain);
    if (D < 0) return -1;
    if (!in) { set_err(h, "ft8rx_ddc_host: in is NULL"); return -1; }
    ENTER(h);
    if (ddc_workspaces(h) || need_staging(h)) return -2;
    const int fmt = sample_fmt(kind);
    const size_t bytes = (size_t)n_streams * (size_t)stream_stride * sf_sample_bytes(fmt);
    if (grow_dev(h, "ft8rx_ddc_host", &h->d_ddc_in, &h->ddc_in_cap, bytes)) return -2;
    if (bytes) HIPCHK(h, hipMemcpyAsync(h->d_ddc_in, in, bytes, hipMemcpyHostToDevice, h->stream));
    if (const int rc = ddc_launch(h, D, h->d_ddc_in, fmt, rate_hz, stream_stride, n_samples, n_out, src, f_dial_hz, gain, h->d_audio, nullptr, f_mixed_hz)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// ---- streaming down-converter.  The index arithmetic is ddc_ring.hpp's.
static void ddc_stream_release(ft8rx_handle* h) {
    ft8rx_handle::DdcStream& s = h->ds;
    release_dev(h, s.d_in); release_dev(h, s.d_out); release_dev(h, s.d_f32); release_dev(h, s.d_outs); release_host(h, s.h_stage);
    release_dev(h, s.d_grid); release_dev(h, s.d_sel);
    const hipEvent_t ev = s.ev;
    s = ft8rx_handle::DdcStream();
    s.ev = ev;
}

// (the bodies of open and push: a pre-stage stream, DESIGN.md section 16.4, opens and feeds the stream behind it through them)
static int ddc_stream_open(ft8rx_handle* h, int kind, int32_t rate_hz, int n_streams, int n_out, const int32_t* src, const double* f_dial_hz,
                           float gain, uint64_t n_origin, int keep_f32, double* f_mixed_hz);
static int ddc_stream_push(ft8rx_handle* h, const void* in, uint64_t n_new, int on_device, uint64_t* m_produced);

// while a pre-stage stream (section 16.4) is open, `ds` is the stage behind it: the plain entries and the one-shots refuse
static int pre_refuse_open(ft8rx_handle* h, const char* who) {
    if (!h->ps.open) return 0;
    set_err(h, "%s: a %s stream is open on this handle (%s_stream_close)", who, h->ps.st.name, h->ps.st.entry);
    return -1;
}
static int pre_refuse_other(ft8rx_handle* h, const char* who, const char* verb) {
    if (!h->ps.open) return 0;
    set_err(h, "%s: the open stream is a %s stream (%s_stream_%s)", who, h->ps.st.name, h->ps.st.entry, verb);
    return -1;
}

int ft8rx_ddc_stream_open(ft8rx_handle* h, int kind, int32_t rate_hz, int n_streams, int n_out, const int32_t* src, const double* f_dial_hz,
                          float gain, uint64_t n_origin, int keep_f32, double* f_mixed_hz) {
    if (!h) return -1;
    if (pre_refuse_open(h, "ft8rx_ddc_stream_open")) return -1;
    return ddc_stream_open(h, kind, rate_hz, n_streams, n_out, src, f_dial_hz, gain, n_origin, keep_f32, f_mixed_hz);
}
static int ddc_stream_open(ft8rx_handle* h, int kind, int32_t rate_hz, int n_streams, int n_out, const int32_t* src, const double* f_dial_hz,
                           float gain, uint64_t n_origin, int keep_f32, double* f_mixed_hz) {
    if (h->ds.open) { set_err(h, "ft8rx_ddc_stream_open: a stream is open on this handle already (ft8rx_ddc_stream_close)"); return -1; }
    const int D = ddc_check(h, "ft8rx_ddc_stream_open", kind, rate_hz, n_streams, 0, 0, n_out, src, f_dial_hz, gain);
    if (D < 0) return -1;
    if (n_origin % (uint64_t)(DDC_TO * D) != 0 || n_origin > ((uint64_t)1 << 62)) {
        set_err(h, "ft8rx_ddc_stream_open: n_origin %llu is not a multiple of %d (1008 D)", (unsigned long long)n_origin, DDC_TO * D); return -1;
    }
    ENTER(h);
    if (ddc_workspaces(h)) return -2;
    ft8rx_handle::DdcStream& s = h->ds;
    if (!s.ev) HIPCHK(h, hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    const int fmt = sample_fmt(kind);
    const size_t sb = sf_sample_bytes(fmt), cap = (size_t)ddcring::in_capacity(D);
    char* d_in = nullptr;
    int rc = dalloc(h, &d_in, (size_t)n_streams * cap * sb);
    s.d_in = d_in;
    if (!rc) rc = dalloc(h, &s.d_out, (size_t)n_out * ddcring::OUT_RING);
    if (!rc && keep_f32) rc = dalloc(h, &s.d_f32, (size_t)n_out * ddcring::OUT_RING);
    if (!rc) rc = dalloc(h, &s.d_outs, (size_t)n_out);
    if (!rc) rc = halloc(h, &s.h_stage, (size_t)n_streams * (size_t)rate_hz * sb);
    if (rc) { ddc_stream_release(h); return -2; }
    std::vector<DdcOut> outs((size_t)n_out);
    ddc_table(outs.data(), rate_hz, n_out, src, f_dial_hz, f_mixed_hz);
    hipError_t e = hipMemcpyAsync(s.d_outs, outs.data(), sizeof(DdcOut) * (size_t)n_out, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.d_out, 0, sizeof(int16_t) * (size_t)n_out * ddcring::OUT_RING, h->stream);
    if (e == hipSuccess && s.d_f32) e = hipMemsetAsync(s.d_f32, 0, sizeof(float) * (size_t)n_out * ddcring::OUT_RING, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);      // the table is a pageable vector of this call
    if (e != hipSuccess) { set_err(h, "ft8rx_ddc_stream_open: %s", hipGetErrorString(e)); ddc_stream_release(h); return -2; }
    s.fmt = fmt; s.D = D; s.rate = rate_hz; s.n_streams = n_streams; s.n_out = n_out; s.cap = (int64_t)cap;
    s.scale = gain * sf_real_gain(fmt);
    s.f32_frames = keep_f32 == FT8RX_DDC_KEEP_F32_FRAMES;
    s.n_origin = (int64_t)n_origin; s.pushed = 0; s.tiles = s.n_origin / (DDC_TO * D);
    s.open = true;
    return 0;
}

int ft8rx_ddc_stream_push(ft8rx_handle* h, const void* in, uint64_t n_new, int on_device, uint64_t* m_produced) {
    if (!h) return -1;
    if (pre_refuse_other(h, "ft8rx_ddc_stream_push", "push")) return -1;
    return ddc_stream_push(h, in, n_new, on_device, m_produced);
}
static int ddc_stream_push(ft8rx_handle* h, const void* in, uint64_t n_new, int on_device, uint64_t* m_produced) {
    ft8rx_handle::DdcStream& s = h->ds;
    if (!s.open) { set_err(h, "ft8rx_ddc_stream_push: no stream is open (ft8rx_ddc_stream_open)"); return -1; }
    if (n_new < 1 || n_new > (uint64_t)s.rate) { set_err(h, "ft8rx_ddc_stream_push: n_new %llu outside [1, %d] (one second)", (unsigned long long)n_new, (int)s.rate); return -1; }
    const size_t sb = sf_sample_bytes(s.fmt);
    if (!in || (on_device && ((uintptr_t)in % sb) != 0)) { set_err(h, "ft8rx_ddc_stream_push: in is NULL or not aligned to a sample"); return -1; }
    // (no ENTER: a push touches the stream's own rings only, on the main stream; batches in flight read neither)
    HIPCHK(h, hipSetDevice(h->device));
    const char* from = (const char*)in;
    if (!on_device) {                                    // through the page-locked buffer, once the previous push's copies have left it
        HIPCHK(h, hipEventSynchronize(s.ev));
        memcpy(s.h_stage, in, (size_t)s.n_streams * (size_t)n_new * sb);
        from = s.h_stage;
    }
    const hipMemcpyKind dir = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const ddcring::Split sp = ddcring::split(s.pushed, (int64_t)n_new, s.cap);
    for (int i = 0; i < s.n_streams; i++) {              // at most two copies per stream: up to the ring's end, then from its start
        char* ring = (char*)s.d_in + (size_t)i * (size_t)s.cap * sb;
        const char* chunk = from + (size_t)i * (size_t)n_new * sb;
        HIPCHK(h, hipMemcpyAsync(ring + (size_t)sp.pos * sb, chunk, (size_t)sp.first * sb, dir, h->stream));
        if (sp.second) HIPCHK(h, hipMemcpyAsync(ring, chunk + (size_t)sp.first * sb, (size_t)sp.second * sb, dir, h->stream));
    }
    if (!on_device) HIPCHK(h, hipEventRecord(s.ev, h->stream));
    s.pushed += (int64_t)n_new;
    const int64_t n_end = s.n_origin + s.pushed, done = ddcring::tiles_done(s.n_origin, n_end, s.D);
    const int n_tiles = (int)(done - s.tiles);           // at most 12000 / 1008 + 1
    if (n_tiles > 0) {
        const unsigned grid = (unsigned)s.n_out * (unsigned)n_tiles;
#define DDC_GO(DD) k_ddc_stream<DD><<<grid, DDC_NT, 0, h->stream>>>(s.d_in, s.fmt, (unsigned long long)s.cap, (long long)s.n_origin, (long long)n_end, \
                                                                   s.d_outs, (long long)s.tiles, n_tiles, s.scale, (int)ddcring::OUT_RING, s.d_out, s.d_f32)
        switch (s.D) { case 1: DDC_GO(1); break; case 2: DDC_GO(2); break; case 4: DDC_GO(4); break; case 8: DDC_GO(8); break; default: DDC_GO(16); }
#undef DDC_GO
        HIPCHK(h, hipGetLastError());
        if (s.d_grid) {                                  // the rows these tiles complete, behind them on the same stream (section 16.5)
            const int64_t m_origin = s.n_origin / s.D;
            const ddcgrid::Hops hp = ddcgrid::completed(s.tiles * DDC_TO, done * DDC_TO, s.g_p0, m_origin, s.g_rows);
            if (hp.end > hp.first) {
                const dim3 g((unsigned)(hp.end - hp.first), (unsigned)s.n_out);
                const int slot0 = (int)ddcgrid::window_slot(hp.first, s.g_p0), nz0 = (int)ddcgrid::zero_prefix(hp.first, s.g_p0, m_origin);
                const int row0 = (int)ddcgrid::row_slot(hp.first, s.g_rows);
                if (s.f32_frames)       // a stream of float frames: the rows of the unrounded ring
                    k_grid_stream<SpecLoadRingF32><<<g, SPEC_NT, 0, h->stream>>>(s.d_f32, (int)ddcring::OUT_RING, slot0, nz0, s.d_grid, s.g_rows, row0, h->T);
                else
                    k_grid_stream<SpecLoadRing><<<g, SPEC_NT, 0, h->stream>>>(s.d_out, (int)ddcring::OUT_RING, slot0, nz0, s.d_grid, s.g_rows, row0, h->T);
                HIPCHK(h, hipGetLastError());
            }
        }
        s.tiles = done;
    }
    if (m_produced) *m_produced = (uint64_t)(s.tiles * DDC_TO);
    return 0;
}

// the two frame entries: the int16 ring into int16 frames, or (f32) the float32 ring into float32 frames; d_audio NULL = the staging buffer
static int ddc_stream_frame(ft8rx_handle* h, const char* who, uint64_t m_first_u, int n_have, void* d_audio, bool f32) {
    if (!h) return -1;
    ft8rx_handle::DdcStream& s = h->ds;
    if (!s.open) { set_err(h, "%s: no stream is open (ft8rx_ddc_stream_open)", who); return -1; }
    if (f32 && !s.d_f32) { set_err(h, "%s: the stream was opened without the float32 ring (keep_f32)", who); return -1; }
    if (n_have < 0 || n_have > FT8RX_NSAMP) { set_err(h, "%s: n_have %d outside [0, %d]", who, n_have, FT8RX_NSAMP); return -1; }
    const int64_t m_first = (int64_t)m_first_u;          // two's complement: a negative index lies before index 0
    if (m_first < -((int64_t)1 << 62) || m_first > ((int64_t)1 << 62)) { set_err(h, "%s: m_first out of range", who); return -1; }
    const int64_t m_origin = s.n_origin / s.D, m_done = s.tiles * DDC_TO;
    if (!ddcring::held(m_first, n_have, m_origin, m_done).ok) {
        set_err(h, "%s: outputs from %lld on have left the ring (it holds %lld .. %lld)", who, (long long)(m_first > m_origin ? m_first : m_origin),
                (long long)(m_done - ddcring::OUT_RING), (long long)m_done);
        return -1;
    }
    if (f32 && ((uintptr_t)d_audio % sizeof(float)) != 0) { set_err(h, "%s: d_audio is not aligned to a sample", who); return -1; }
    ENTER(h);                                            // a batch in flight may still read the staging audio
    if (!d_audio) { if (need_staging(h, f32 ? 4 : 2, false)) return -2; d_audio = staging_of(h, f32 ? 4 : 2, false); }
    const dim3 g((FT8RX_NSAMP + 255) / 256, (unsigned)s.n_out);
    if (f32) k_ddc_gather_f32<<<g, 256, 0, h->stream>>>(s.d_f32, (int)ddcring::OUT_RING, (long long)m_first, n_have, (long long)m_origin, (long long)m_done, (float*)d_audio);
    else k_ddc_gather<<<g, 256, 0, h->stream>>>(s.d_out, (int)ddcring::OUT_RING, (long long)m_first, n_have, (long long)m_origin, (long long)m_done, (int16_t*)d_audio);
    HIPCHK(h, hipGetLastError());
    return 0;
}
int ft8rx_ddc_stream_frame(ft8rx_handle* h, uint64_t m_first, int n_have, int16_t* d_audio) {
    return ddc_stream_frame(h, "ft8rx_ddc_stream_frame", m_first, n_have, d_audio, false);
}
int ft8rx_ddc_stream_frame_f32(ft8rx_handle* h, uint64_t m_first, int n_have, float* d_audio) {
    return ddc_stream_frame(h, "ft8rx_ddc_stream_frame_f32", m_first, n_have, d_audio, true);
}

// Frames of either length for chosen channels: the argument checks are ddc_frames.hpp's, what the ring holds
// ddc_ring.hpp's, as in the entries above.  The channel table is the stream's: allocated at the stream's first call here (max_frames
// entries: the longest list a call may give), uploaded when the list differs from the last call's, released with the stream.
static int ft4_workspaces(ft8rx_handle* h);
int ft8rx_ddc_stream_frames(ft8rx_handle* h, uint64_t m_first_u, int n_have, int frame_len, const int32_t* channels, int n_sel, int16_t* d_audio) {
    static const char* who = "ft8rx_ddc_stream_frames";
    if (!h) return -1;
    ft8rx_handle::DdcStream& s = h->ds;
    if (!s.open) { set_err(h, "%s: no stream is open (ft8rx_ddc_stream_open)", who); return -1; }
    const ddcframes::Verdict v = ddcframes::check(frame_len, n_have, channels, n_sel, s.n_out, h->max_frames);
    if (v.bad) {
        char msg[256];
        ddcframes::describe(msg, sizeof msg, who, v, frame_len, n_have, channels, n_sel, s.n_out, h->max_frames);
        set_err(h, "%s", msg);
        return -1;
    }
    const int64_t m_first = (int64_t)m_first_u;          // two's complement: a negative index lies before index 0
    if (m_first < -((int64_t)1 << 62) || m_first > ((int64_t)1 << 62)) { set_err(h, "%s: m_first out of range", who); return -1; }
    const int64_t m_origin = s.n_origin / s.D, m_done = s.tiles * DDC_TO;
    if (!ddcring::held(m_first, n_have, m_origin, m_done).ok) {
        set_err(h, "%s: outputs from %lld on have left the ring (it holds %lld .. %lld)", who, (long long)(m_first > m_origin ? m_first : m_origin),
                (long long)(m_done - ddcring::OUT_RING), (long long)m_done);
        return -1;
    }
    ENTER(h);                                            // a batch in flight may still read the frames' buffer
    if (!d_audio) {
        if (frame_len == FT8RX_FT4_NSAMP) { if (const int rc = ft4_workspaces(h)) return rc; d_audio = h->ft4.d_audio; }
        else { if (need_staging(h)) return -2; d_audio = h->d_audio; }
    }
    if (!s.d_sel && dalloc(h, &s.d_sel, (size_t)h->max_frames)) return -2;
    if (ddcframes::differs(s.sel.data(), (int)s.sel.size(), channels, n_sel)) {
        s.sel.resize((size_t)n_sel);
        for (int i = 0; i < n_sel; i++) s.sel[i] = channels ? channels[i] : i;
        // after the gathers that still read the old table, and complete before this call returns: the list is a pageable vector
        const hipError_t e = hipMemcpyAsync(s.d_sel, s.sel.data(), sizeof(int32_t) * (size_t)n_sel, hipMemcpyHostToDevice, h->stream);
        const hipError_t e2 = hipStreamSynchronize(h->stream);
        if (e != hipSuccess || e2 != hipSuccess) { s.sel.clear(); set_err(h, "%s: %s", who, hipGetErrorString(e != hipSuccess ? e : e2)); return -2; }
    }
    const dim3 g((unsigned)(frame_len + 255) / 256, (unsigned)n_sel);
    k_ddc_gather_sel<<<g, 256, 0, h->stream>>>(s.d_out, (int)ddcring::OUT_RING, s.d_sel, s.n_out, (long long)m_first, n_have, (long long)m_origin,
                                               (long long)m_done, frame_len, d_audio);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int ft8rx_ddc_stream_read(ft8rx_handle* h, uint64_t m_first_u, int n, int16_t* y_i16, float* y_f32) {
    if (!h) return -1;
    ft8rx_handle::DdcStream& s = h->ds;
    if (!s.open) { set_err(h, "ft8rx_ddc_stream_read: no stream is open (ft8rx_ddc_stream_open)"); return -1; }
    const int64_t m_first = (int64_t)m_first_u, m_origin = s.n_origin / s.D, m_done = s.tiles * DDC_TO;
    if (n < 1 || m_first < m_origin || m_first + n > m_done || m_first < m_done - ddcring::OUT_RING) {
        set_err(h, "ft8rx_ddc_stream_read: outputs [%lld, %lld) are not all in the ring (it holds %lld .. %lld)", (long long)m_first, (long long)(m_first + n),
                (long long)(m_done - ddcring::OUT_RING > m_origin ? m_done - ddcring::OUT_RING : m_origin), (long long)m_done);
        return -1;
    }
    if (y_f32 && !s.d_f32) { set_err(h, "ft8rx_ddc_stream_read: the stream was opened without the float32 copy (keep_f32)"); return -1; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int64_t pos = ddcring::out_pos(m_first), first = n < ddcring::OUT_RING - pos ? n : ddcring::OUT_RING - pos;
    for (int j = 0; j < s.n_out; j++) {
        const size_t row = (size_t)j * ddcring::OUT_RING;
        if (y_i16) {
            HIPCHK(h, hipMemcpy(y_i16 + (size_t)j * n, s.d_out + row + pos, sizeof(int16_t) * (size_t)first, hipMemcpyDeviceToHost));
            if (first < n) HIPCHK(h, hipMemcpy(y_i16 + (size_t)j * n + first, s.d_out + row, sizeof(int16_t) * (size_t)(n - first), hipMemcpyDeviceToHost));
        }
        if (y_f32) {
            HIPCHK(h, hipMemcpy(y_f32 + (size_t)j * n, s.d_f32 + row + pos, sizeof(float) * (size_t)first, hipMemcpyDeviceToHost));
            if (first < n) HIPCHK(h, hipMemcpy(y_f32 + (size_t)j * n + first, s.d_f32 + row, sizeof(float) * (size_t)(n - first), hipMemcpyDeviceToHost));
        }
    }
    return 0;
}

int ft8rx_ddc_stream_info(ft8rx_handle* h, uint64_t* in_capacity, uint64_t* out_capacity, uint64_t* n_pushed, uint64_t* m_produced) {
    if (!h) return -1;
    const ft8rx_handle::DdcStream& s = h->ds;
    if (!s.open) { set_err(h, "ft8rx_ddc_stream_info: no stream is open (ft8rx_ddc_stream_open)"); return -1; }
    if (in_capacity) *in_capacity = (uint64_t)s.cap;
    if (out_capacity) *out_capacity = (uint64_t)ddcring::OUT_RING;
    if (n_pushed) *n_pushed = (uint64_t)s.pushed;
    if (m_produced) *m_produced = (uint64_t)(s.tiles * DDC_TO);
    return 0;
}

// ---- the spectrogram stage behind the stream.  The index arithmetic is ddc_grid_ring.hpp's.  The three entries
// serve a plain stream and the stage behind a pre-stage stream alike (as ft8rx_ddc_stream_frame / _read / _info do).
int ft8rx_ddc_stream_grid_open(ft8rx_handle* h, int hop_phase, int n_rows) {
    if (!h) return -1;
    ft8rx_handle::DdcStream& s = h->ds;
    if (!s.open) { set_err(h, "ft8rx_ddc_stream_grid_open: no stream is open (ft8rx_ddc_stream_open)"); return -1; }
    if (s.d_grid) { set_err(h, "ft8rx_ddc_stream_grid_open: the grid is open already (p0 %d, %d rows)", s.g_p0, s.g_rows); return -1; }
    const int64_t pushed = h->ps.open ? h->ps.pushed : s.pushed;
    if (pushed) { set_err(h, "ft8rx_ddc_stream_grid_open: %lld samples have been pushed already (open the grid before the first push)", (long long)pushed); return -1; }
    if (hop_phase < 0 || hop_phase >= ddcgrid::HOP) { set_err(h, "ft8rx_ddc_stream_grid_open: hop_phase %d outside [0, %d)", hop_phase, (int)ddcgrid::HOP); return -1; }
    if (n_rows < ddcgrid::MIN_ROWS || n_rows > ddcgrid::MAX_ROWS) {
        set_err(h, "ft8rx_ddc_stream_grid_open: n_rows %d outside [%d, %d]", n_rows, (int)ddcgrid::MIN_ROWS, (int)ddcgrid::MAX_ROWS); return -1;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (dalloc(h, &s.d_grid, (size_t)s.n_out * (size_t)n_rows * FT8RX_GRID_COLS)) return -2;
    s.g_p0 = hop_phase; s.g_rows = n_rows;
    return 0;
}

int ft8rx_ddc_stream_grid_info(ft8rx_handle* h, uint64_t* q_first_held, uint64_t* q_next, int32_t* cols, int32_t* n_rows) {
    if (!h) return -1;
    const ft8rx_handle::DdcStream& s = h->ds;
    if (!s.open || !s.d_grid) { set_err(h, "ft8rx_ddc_stream_grid_info: no grid is open (ft8rx_ddc_stream_grid_open)"); return -1; }
    const ddcgrid::Held hd = ddcgrid::held(s.tiles * DDC_TO, s.g_p0, s.n_origin / s.D, s.g_rows);
    if (q_first_held) *q_first_held = (uint64_t)hd.first;
    if (q_next) *q_next = (uint64_t)hd.next;
    if (cols) *cols = FT8RX_GRID_COLS;
    if (n_rows) *n_rows = s.g_rows;
    return 0;
}

int ft8rx_ddc_stream_grid_read(ft8rx_handle* h, uint64_t q_first_u, int n, float* rows) {
    if (!h) return -1;
    const ft8rx_handle::DdcStream& s = h->ds;
    if (!s.open || !s.d_grid) { set_err(h, "ft8rx_ddc_stream_grid_read: no grid is open (ft8rx_ddc_stream_grid_open)"); return -1; }
    if (!rows) { set_err(h, "ft8rx_ddc_stream_grid_read: rows is NULL"); return -1; }
    const ddcgrid::Held hd = ddcgrid::held(s.tiles * DDC_TO, s.g_p0, s.n_origin / s.D, s.g_rows);
    const int64_t q_first = (int64_t)q_first_u;
    if (n < 1 || q_first < hd.first || q_first > hd.next || n > hd.next - q_first) {
        set_err(h, "ft8rx_ddc_stream_grid_read: rows [%lld, %lld) are not all in the grid ring (it holds %lld .. %lld)", (long long)q_first,
                (long long)(q_first + (n > 0 ? n : 0)), (long long)hd.first, (long long)hd.next);
        return -1;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int64_t pos = ddcgrid::row_slot(q_first, s.g_rows), first = n < s.g_rows - pos ? n : s.g_rows - pos;
    for (int j = 0; j < s.n_out; j++) {                  // at most two copies per channel: up to the grid ring's end, then from its start
        const float* ring = s.d_grid + (size_t)j * (size_t)s.g_rows * FT8RX_GRID_COLS;
        float* to = rows + (size_t)j * (size_t)n * FT8RX_GRID_COLS;
        HIPCHK(h, hipMemcpy(to, ring + (size_t)pos * FT8RX_GRID_COLS, sizeof(float) * (size_t)first * FT8RX_GRID_COLS, hipMemcpyDeviceToHost));
        if (first < n) HIPCHK(h, hipMemcpy(to + (size_t)first * FT8RX_GRID_COLS, ring, sizeof(float) * (size_t)(n - first) * FT8RX_GRID_COLS, hipMemcpyDeviceToHost));
    }
    return 0;
}

int ft8rx_ddc_stream_close(ft8rx_handle* h) {
    if (!h) return -1;
    if (pre_refuse_other(h, "ft8rx_ddc_stream_close", "close")) return -1;
    if (!h->ds.open) { set_err(h, "ft8rx_ddc_stream_close: no stream is open"); return -1; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));          // pushes and gathers that still use the rings
    ddc_stream_release(h);
    return 0;
}

// ---------------------------------------------------------------------------- input pre-stages (DESIGN.md sections 16.2 - 16.4)
// The wide pre-decimator (ft8rx_ddc_wide*) and the rational resampler (ft8rx_ddc_rat*) share one host path: a PreStage says what differs.
// The kernels' tiles and the limits, against the pure index arithmetic of ddc_wide_ring.hpp and ddc_rat_ring.hpp
static_assert(ddcwide::PIECE == DDW_JP && ddcwide::LDS_SAMPLES == DDW_LS && ddcwide::TILE_MAX == DDW_TK && DDW_JP % 64 == 0 && DDW_TK == 4 * (DDW_NT / 64),
              "ddc_wide_ring.hpp: the tile of kernels/ddc_wide.hpp");
constexpr bool ddw_tiles_fit() {
    for (int64_t r = 2; r <= ddcwide::MAX_R0; r++)
        if (ddcwide::tile_outputs(r) < 1 || (ddcwide::tile_outputs(r) - 1) * r + DDW_JP > DDW_LS) return false;
    return true;
}
static_assert(ddw_tiles_fit(), "ddc_wide_ring.hpp: a tile's input under one piece of taps fits the LDS image");
static_assert(ddcwide::plan(240000).rate_mid == 48000 && ddcwide::plan(240000).R0 == 5 && ddcwide::plan(64800000).rate_mid == 96000 &&
              ddcwide::plan(129600000).R0 == 675 && ddcwide::plan(192000).rate_mid == 0 && ddcwide::plan(129648000).rate_mid == 0, "ddc_wide_ring.hpp: plan");
static_assert(sizeof(float2) * DDW_LS <= 64 * 1024, "the LDS image is static shared memory");
static_assert(ddcrat::LANE_P == 64 && ddcrat::LANE_TABLE == DDR_TAB && ddcrat::LANE_SAMPLES == DDR_LS_LANE && ddcrat::LANE_TILE == DDR_NT &&
              ddcrat::PIECE == DDR_JP && ddcrat::WAVE_SAMPLES == DDR_LS_WAVE && ddcrat::WAVE_TILE == DDR_TK_WAVE && DDR_JP % 64 == 0 &&
              DDR_TK_WAVE == 4 * (DDR_NT / 64), "ddc_rat_ring.hpp: the tiles of kernels/ddc_rat.hpp");
static_assert(DdrLds<true, true>::BYTES <= 64 * 1024 && DdrLds<true, false>::BYTES <= 64 * 1024, "the LDS image is static shared memory");
static_assert(ddcrat::plan(44100).rate_mid == 48000 && ddcrat::plan(44100).L == 160 && ddcrat::plan(44100).M == 147 &&
              ddcrat::plan(2048000).rate_mid == 192000 && ddcrat::plan(2048000).L == 3 && ddcrat::plan(2048000).M == 32 &&
              ddcrat::plan(20000000).rate_mid == 96000 && ddcrat::plan(48000).rate_mid == 0 && ddcrat::plan(2400000).rate_mid == 0 &&
              ddcrat::plan(900001).rate_mid == 0 && ddcrat::plan(15999).rate_mid == 0, "ddc_rat_ring.hpp: plan");
// a tile of either regime holds at least one output and its inputs fit the LDS image, whatever M / L and P
constexpr bool ddr_tiles_fit() {
    for (int64_t m = 1; m <= ddcrat::MAX_TAPS; m += 7)
        for (int64_t p = 1; p <= ddcrat::LANE_P; p += 9) {
            const int64_t a = ddcrat::tile_fit(DDR_LS_LANE, p, 1, m, DDR_NT), b = ddcrat::tile_fit(DDR_LS_WAVE, DDR_JP, 1, m, DDR_TK_WAVE);
            if (a < 1 || (a - 1) * m + 1 + p > DDR_LS_LANE || b < 1 || (b - 1) * m + 1 + DDR_JP > DDR_LS_WAVE) return false;
        }
    return true;
}
static_assert(ddr_tiles_fit(), "ddc_rat_ring.hpp: a tile's input fits the LDS image");

// The prototype of a rate, designed once per (stage, rate) by the recipe of ddc_design at 85 dB, pass 3200 Hz.
//   wide      h0 at fs = rate, stop rate_mid - 3200 Hz
//   rational  h at fs = rate L, stop min(rate, rate_mid) - 3200 Hz, sum h = L; its length is worked out before it is made
// nullptr: the plan refuses the rate, or the filter is longer than the stage's MAX_TAPS
static const std::vector<float>* pre_taps(int which, int32_t rate_hz) {
    double fs, f_stop, dc = 1.0;
    int64_t most;
    if (which == PRE_WIDE) {
        const ddcwide::Plan p = ddcwide::plan(rate_hz);
        if (!p.rate_mid) return nullptr;
        fs = (double)rate_hz; f_stop = (double)p.rate_mid - 3200.0; most = ddcwide::MAX_TAPS;
    } else {
        const ddcrat::Plan p = ddcrat::plan(rate_hz);
        if (!p.rate_mid) return nullptr;
        fs = (double)rate_hz * (double)p.L; f_stop = (double)(rate_hz < p.rate_mid ? rate_hz : p.rate_mid) - 3200.0; dc = (double)p.L; most = ddcrat::MAX_TAPS;
        if ((85.0 - 7.95) / (2.285 * 2.0 * M_PI * (f_stop - 3200.0) / fs) + 2.0 > (double)most) return nullptr;
    }
    static std::mutex mu;
    static std::map<std::pair<int, int32_t>, std::vector<float>> designed;
    std::lock_guard<std::mutex> lock(mu);
    const std::pair<int, int32_t> key(which, rate_hz);
    auto it = designed.find(key);
    if (it == designed.end()) it = designed.emplace(key, ddc_design(3200.0, f_stop, 85.0, fs, dc)).first;
    return (int64_t)it->second.size() <= most ? &it->second : nullptr;
}

// the front stage of a rate; taps == nullptr: refused
static PreStage pre_plan(int which, int32_t rate_hz) {
    PreStage d;
    d.which = which; d.rate = rate_hz;
    d.name = PRE_NAME[which]; d.entry = PRE_ENTRY[which];
    d.taps = pre_taps(which, rate_hz);
    if (!d.taps) return d;
    d.n_taps = (int)d.taps->size();
    if (which == PRE_WIDE) {
        const ddcwide::Plan p = ddcwide::plan(rate_hz);
        d.rate_mid = (int32_t)p.rate_mid; d.M = (int)p.R0;
        d.H = (int)ddcwide::history(d.n_taps, p.R0); d.tk = (int)ddcwide::tile_outputs(p.R0);
        d.n_max = ddcwide::N_MAX; d.end_max = INT64_MAX;
    } else {
        const ddcrat::Plan p = ddcrat::plan(rate_hz);
        d.rate_mid = (int32_t)p.rate_mid; d.L = (int)p.L; d.M = (int)p.M;
        d.P = (int)ddcrat::phase_taps(d.n_taps, p.L); d.H = (int)ddcrat::history(d.n_taps, p.L); d.tk = (int)ddcrat::tile_outputs(d.n_taps, p.L, p.M);
        d.lane = ddcrat::lane_regime(d.n_taps, p.L);
        d.n_max = ddcrat::N_MAX; d.end_max = 2 * ddcrat::N_MAX;      // a stream ends below 2^53, so that n L stays below 2^62
    }
    return d;
}

int ft8rx_ddc_wide_plan(int32_t rate_hz, int32_t* rate_mid_hz, int32_t* r0) {
    const ddcwide::Plan p = ddcwide::plan(rate_hz);
    if (!p.rate_mid) return -1;
    if (rate_mid_hz) *rate_mid_hz = (int32_t)p.rate_mid;
    if (r0) *r0 = (int32_t)p.R0;
    return 0;
}

int ft8rx_ddc_rat_plan(int32_t rate_hz, int32_t* rate_mid_hz, int32_t* l, int32_t* m, int32_t* n_taps) {
    const PreStage d = pre_plan(PRE_RAT, rate_hz);
    if (!d.taps) return -1;
    if (rate_mid_hz) *rate_mid_hz = d.rate_mid;
    if (l) *l = d.L;
    if (m) *m = d.M;
    if (n_taps) *n_taps = d.n_taps;
    return 0;
}

static int pre_taps_out(int which, int32_t rate_hz, float* taps, int cap) {
    const std::vector<float>* t = pre_taps(which, rate_hz);
    if (!t) return -1;
    for (int i = 0; taps && i < cap && i < (int)t->size(); i++) taps[i] = (*t)[i];
    return (int)t->size();
}
int ft8rx_ddc_wide_taps(int32_t rate_hz, float* taps, int cap) { return pre_taps_out(PRE_WIDE, rate_hz, taps, cap); }
int ft8rx_ddc_rat_taps(int32_t rate_hz, float* taps, int cap) { return pre_taps_out(PRE_RAT, rate_hz, taps, cap); }

// the argument checks every entry shares -> 0 and the stage in d, or -1 with the error text
static int pre_check(ft8rx_handle* h, const char* who, int which, PreStage& d, int kind, int32_t rate_hz, int n_out, const double* f_dial_hz, float gain) {
    d = pre_plan(which, rate_hz);
    if (!sf_kind_in(PRE_KINDS[which], kind)) {
        if (which == PRE_WIDE) set_err(h, "%s: kind %d is not one of FT8RX_WIDE_REAL_I16 .. FT8RX_WIDE_IQ_I8", who, kind);
        else set_err(h, "%s: kind %d is not one of FT8RX_DDC_REAL_I16 .. FT8RX_DDC_IQ_F32, FT8RX_WIDE_IQ_U8, FT8RX_WIDE_IQ_I8", who, kind);
        return -1;
    }
    if (!d.taps) {
        if (which == PRE_WIDE) set_err(h, "%s: rate_hz %d is not a multiple of 48000 in [240000, 129600000] with rate_hz / rate_mid <= 1350", who, (int)rate_hz);
        else set_err(h, "%s: rate_hz %d is not taken: outside [16000, 129600000], a rate of ft8rx_ddc or ft8rx_ddc_wide, L > 320 or more than 8448 taps", who, (int)rate_hz);
        return -1;
    }
    if (n_out < 1 || n_out > h->max_frames || n_out > 65535) { set_err(h, "%s: n_out %d outside [1, %d] (max_frames; at most 65535)", who, n_out, h->max_frames); return -1; }
    if (!f_dial_hz) { set_err(h, "%s: f_dial_hz is NULL", who); return -1; }
    for (int j = 0; j < n_out; j++)
        if (!(f_dial_hz[j] >= -0.5 * rate_hz && f_dial_hz[j] < 0.5 * rate_hz)) { set_err(h, "%s: f_dial_hz[%d] = %g outside [-rate_hz / 2, rate_hz / 2)", who, j, f_dial_hz[j]); return -1; }
    if (!(fabsf(gain) <= 3.0e38f)) { set_err(h, "%s: gain is not finite", who); return -1; }
    return 0;
}

// One channel's table.  Wide: W[j] = h0[j] e^{-2 pi i (w0 j mod 2^32) / 2^32}, [n_taps].  Rational: by phase, T[phi][i] = h[phi + i L]
// e^{+2 pi i (w0 i mod 2^32) / 2^32}, [L][P], zero from N on.  Both in double, rounded once.
static void pre_fill_wide(const std::vector<float>& h0, uint32_t w0, float2* tab) {
    for (size_t j = 0; j < h0.size(); j++) {
        const double a = -(double)(uint32_t)(w0 * (uint32_t)j) * (M_PI / 2147483648.0);
        tab[j] = make_float2((float)((double)h0[j] * cos(a)), (float)((double)h0[j] * sin(a)));
    }
}
static void pre_fill_rat(const std::vector<float>& hp, size_t L, size_t P, uint32_t w0, float2* tab) {
    const size_t N = hp.size();
    for (size_t i = 0; i < P; i++) {
        const double a = (double)(uint32_t)(w0 * (uint32_t)i) * (M_PI / 2147483648.0), ca = cos(a), sa = sin(a);
        for (size_t phi = 0; phi < L && phi + i * L < N; phi++) {
            const double hv = (double)hp[phi + i * L];
            tab[phi * P + i] = make_float2((float)(hv * ca), (float)(hv * sa));
        }
    }
}
// per channel: the frequency word w0, its table, the dial left for the stage behind (f_dial - f0, about -3000 Hz) and f0 itself, both
// taken into [-rate / 2, rate / 2)
struct PreTables { std::vector<float2> tab; std::vector<uint32_t> w0s; std::vector<double> dial_mid, f0s; };
static void pre_tables(const PreStage& d, int n_out, const double* f_dial_hz, PreTables& t) {
    const size_t per = d.which == PRE_WIDE ? (size_t)d.n_taps : (size_t)d.L * (size_t)d.P;
    const double rate = (double)d.rate;
    t.tab.assign((size_t)n_out * per, make_float2(0.0f, 0.0f)); t.w0s.resize((size_t)n_out); t.dial_mid.resize((size_t)n_out); t.f0s.resize((size_t)n_out);
    for (int c = 0; c < n_out; c++) {
        const double r = nearbyint((f_dial_hz[c] + 3000.0) / rate * 4294967296.0);
        const uint32_t w0 = (uint32_t)((long long)r & 0xffffffffLL);
        double f0 = (double)w0 * rate / 4294967296.0;
        if (f0 >= 0.5 * d.rate) f0 -= rate;
        double dm = f_dial_hz[c] - f0;
        dm -= rate * nearbyint(dm / rate);
        t.w0s[c] = w0; t.f0s[c] = f0; t.dial_mid[c] = dm;
        if (d.which == PRE_WIDE) pre_fill_wide(*d.taps, w0, t.tab.data() + (size_t)c * per);
        else pre_fill_rat(*d.taps, (size_t)d.L, (size_t)d.P, w0, t.tab.data() + (size_t)c * per);
    }
}
// what the caller sees as mixed: f0 + the dial the stage behind really mixed, in [-rate / 2, rate / 2)
static void pre_mixed(int32_t rate_hz, int n_out, const std::vector<double>& f0s, double* f_mixed_hz) {
    for (int c = 0; f_mixed_hz && c < n_out; c++) {
        double f = f0s[c] + f_mixed_hz[c];
        if (f >= 0.5 * rate_hz) f -= (double)rate_hz;
        if (f < -0.5 * rate_hz) f += (double)rate_hz;
        f_mixed_hz[c] = f;
    }
}

// The two launches (with_bool: a run-time bool as a template argument).
// One call: in = n_samples samples of format `fmt` -> mid [n_out][n_mid]
static void pre_launch(ft8rx_handle* h, const PreStage& d, const void* d_in, int fmt, long long n_samples, const float2* tab, const uint32_t* w0s,
                       int n_out, long long n_mid, float2* mid) {
    const dim3 grid((unsigned)((n_mid + d.tk - 1) / d.tk), (unsigned)n_out);
    const float g0 = sf_real_gain(fmt);
    with_bool(sf_is_iq(fmt), [&](auto iq) {
        constexpr bool IQ = decltype(iq)::value;
        if (d.which == PRE_WIDE) k_ddc_pre<IQ><<<grid, DDW_NT, 0, h->stream>>>(d_in, fmt, n_samples, tab, w0s, d.n_taps, d.M, d.tk, g0, n_mid, mid);
        else with_bool(d.lane, [&](auto lane) {
            k_ddc_rat<IQ, decltype(lane)::value><<<grid, DDR_NT, 0, h->stream>>>(d_in, fmt, n_samples, tab, w0s, (d.n_taps - 1) / 2, d.L, d.M, d.P, d.tk, g0, n_mid, mid);
        });
    });
}
// The stream: intermediate samples k_done .. k_done + n_k - 1 of every channel from the history and the chunk [n_start, n_end) -> s.d_mid
static void pre_launch_stream(ft8rx_handle* h, const ft8rx_handle::PreStream& s, const void* chunk, long long n_start, long long n_end, int n_k) {
    const PreStage& d = s.st;
    const dim3 grid((unsigned)((n_k + d.tk - 1) / d.tk), (unsigned)s.n_out);
    const int p_last = s.pushed ? (int)ddcpre::hist_pos(n_start - 1, s.n_origin, d.H) : 0;
    const long long n_origin = s.n_origin, k_first = s.k_done;
    const float g0 = sf_real_gain(s.fmt);
    with_bool(sf_is_iq(s.fmt), [&](auto iq) {
        constexpr bool IQ = decltype(iq)::value;
        if (d.which == PRE_WIDE)
            k_ddc_pre_stream<IQ><<<grid, DDW_NT, 0, h->stream>>>(s.d_hist, d.H, p_last, chunk, s.fmt, n_origin, n_start, n_end, s.d_tab, s.d_w0, d.n_taps, d.M, d.tk,
                                                                 g0, k_first, n_k, s.d_mid);
        else with_bool(d.lane, [&](auto lane) {
            k_ddc_rat_stream<IQ, decltype(lane)::value><<<grid, DDR_NT, 0, h->stream>>>(s.d_hist, d.H, p_last, chunk, s.fmt, n_origin, n_start, n_end, s.d_tab, s.d_w0,
                                                                                       (d.n_taps - 1) / 2, d.L, d.M, d.P, d.tk, g0, k_first, n_k, s.d_mid);
        });
    });
}

// the one-shot behind its checks: the pre-stage into the handle's intermediate buffer, then k_ddc<D> on it with one stream per output
static int pre_run(ft8rx_handle* h, const char* who, const PreStage& d, const void* d_in, int fmt, uint64_t n_samples, int n_out, const double* f_dial_hz,
                   float gain, int16_t* d_audio, float* d_audio_f32, double* f_mixed_hz) {
    const int D = d.rate_mid / 12000;
    const int64_t n_mid = ddcpre::mid_count((int64_t)n_samples, d.n_taps, d.L, d.M, (int64_t)FT8RX_NSAMP * D);
    PreTables t;
    std::vector<double> fm((size_t)n_out);
    pre_tables(d, n_out, f_dial_hz, t);
    if (grow_dev(h, who, &h->d_pre_tab, &h->pre_tab_cap, sizeof(float2) * t.tab.size()) ||
        grow_dev(h, who, &h->d_pre_w0, &h->pre_w0_cap, sizeof(uint32_t) * t.w0s.size()) ||
        grow_dev(h, who, &h->d_pre_mid, &h->pre_mid_cap, sizeof(float2) * (size_t)n_out * (size_t)n_mid)) return -2;
    // the tables are pageable vectors of this call, and an earlier call's kernel may still read the device copies
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(h->d_pre_tab, t.tab.data(), sizeof(float2) * t.tab.size(), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_pre_w0, t.w0s.data(), sizeof(uint32_t) * t.w0s.size(), hipMemcpyHostToDevice));
    pre_launch(h, d, d_in, fmt, (long long)n_samples, (const float2*)h->d_pre_tab, (const uint32_t*)h->d_pre_w0, n_out, (long long)n_mid, (float2*)h->d_pre_mid);
    HIPCHK(h, hipGetLastError());
    std::vector<int32_t> src((size_t)n_out);
    for (int j = 0; j < n_out; j++) src[j] = j;
    if (const int rc = ddc_launch(h, D, h->d_pre_mid, SF_IQ_F32, d.rate_mid, (uint64_t)n_mid, (uint64_t)n_mid, n_out, src.data(), t.dial_mid.data(),
                                  gain, d_audio, d_audio_f32, fm.data())) return rc;
    if (f_mixed_hz) { for (int j = 0; j < n_out; j++) f_mixed_hz[j] = fm[j]; pre_mixed(d.rate, n_out, t.f0s, f_mixed_hz); }
    return 0;
}

static int pre_check_oneshot(ft8rx_handle* h, const char* who, int which, PreStage& d, int kind, int32_t rate_hz, uint64_t n_samples, int n_out,
                             const double* f_dial_hz, float gain) {
    if (pre_check(h, who, which, d, kind, rate_hz, n_out, f_dial_hz, gain) < 0) return -1;
    if (n_samples > (uint64_t)15 * (uint64_t)rate_hz) { set_err(h, "%s: n_samples %llu > %llu (15 s at rate_hz)", who, (unsigned long long)n_samples, 15ull * (unsigned long long)rate_hz); return -1; }
    return pre_refuse_open(h, who);
}

// the device entry (d_in on the device; d_audio: NULL = the staging buffer) and the host entry
static int pre_oneshot(ft8rx_handle* h, const char* who, int which, const void* d_in, int kind, int32_t rate_hz, uint64_t n_samples, int n_out,
                       const double* f_dial_hz, float gain, int16_t* d_audio, float* d_audio_f32, double* f_mixed_hz) {
    if (!h) return -1;
    PreStage d;
    if (pre_check_oneshot(h, who, which, d, kind, rate_hz, n_samples, n_out, f_dial_hz, gain)) return -1;
    const int fmt = sample_fmt(kind);
    if (!d_in || ((uintptr_t)d_in % sf_sample_bytes(fmt)) != 0) { set_err(h, "%s: d_in is NULL or not aligned to a sample", who); return -1; }
    ENTER(h);
    if (ddc_workspaces(h)) return -2;
    if (!d_audio) { if (need_staging(h)) return -2; d_audio = h->d_audio; }
    return pre_run(h, who, d, d_in, fmt, n_samples, n_out, f_dial_hz, gain, d_audio, d_audio_f32, f_mixed_hz);
}
static int pre_oneshot_host(ft8rx_handle* h, const char* who, int which, const void* in, int kind, int32_t rate_hz, uint64_t n_samples, int n_out,
                            const double* f_dial_hz, float gain, double* f_mixed_hz) {
    if (!h) return -1;
    PreStage d;
    if (pre_check_oneshot(h, who, which, d, kind, rate_hz, n_samples, n_out, f_dial_hz, gain)) return -1;
    if (!in) { set_err(h, "%s: in is NULL", who); return -1; }
    ENTER(h);
    if (ddc_workspaces(h) || need_staging(h)) return -2;
    const int fmt = sample_fmt(kind);
    const size_t bytes = (size_t)n_samples * sf_sample_bytes(fmt);
    if (grow_dev(h, who, &h->d_ddc_in, &h->ddc_in_cap, bytes)) return -2;      // the input staging of ft8rx_ddc_host
    if (bytes) HIPCHK(h, hipMemcpyAsync(h->d_ddc_in, in, bytes, hipMemcpyHostToDevice, h->stream));
    if (const int rc = pre_run(h, who, d, h->d_ddc_in, fmt, n_samples, n_out, f_dial_hz, gain, h->d_audio, nullptr, f_mixed_hz)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int ft8rx_ddc_wide(ft8rx_handle* h, const void* d_in, int kind, int32_t rate_hz, uint64_t n_samples, int n_out, const double* f_dial_hz, float gain,
                   int16_t* d_audio, float* d_audio_f32, double* f_mixed_hz) {
    return pre_oneshot(h, "ft8rx_ddc_wide", PRE_WIDE, d_in, kind, rate_hz, n_samples, n_out, f_dial_hz, gain, d_audio, d_audio_f32, f_mixed_hz);
}
int ft8rx_ddc_rat(ft8rx_handle* h, const void* d_in, int kind, int32_t rate_hz, uint64_t n_samples, int n_out, const double* f_dial_hz, float gain,
                  int16_t* d_audio, float* d_audio_f32, double* f_mixed_hz) {
    return pre_oneshot(h, "ft8rx_ddc_rat", PRE_RAT, d_in, kind, rate_hz, n_samples, n_out, f_dial_hz, gain, d_audio, d_audio_f32, f_mixed_hz);
}
int ft8rx_ddc_wide_host(ft8rx_handle* h, const void* in, int kind, int32_t rate_hz, uint64_t n_samples, int n_out, const double* f_dial_hz, float gain,
                        double* f_mixed_hz) {
    return pre_oneshot_host(h, "ft8rx_ddc_wide_host", PRE_WIDE, in, kind, rate_hz, n_samples, n_out, f_dial_hz, gain, f_mixed_hz);
}
int ft8rx_ddc_rat_host(ft8rx_handle* h, const void* in, int kind, int32_t rate_hz, uint64_t n_samples, int n_out, const double* f_dial_hz, float gain,
                       double* f_mixed_hz) {
    return pre_oneshot_host(h, "ft8rx_ddc_rat_host", PRE_RAT, in, kind, rate_hz, n_samples, n_out, f_dial_hz, gain, f_mixed_hz);
}

// ---- the pre-stage stream: the stage on a continuous stream, in front of the streaming down-converter (section 16.1), which it opens,
// feeds on the device and closes.  The index arithmetic is ddc_pre_ring.hpp's.
static void pre_stream_release(ft8rx_handle* h) {
    ft8rx_handle::PreStream& s = h->ps;
    release_dev(h, s.d_hist); release_dev(h, s.d_chunk); release_dev(h, s.d_mid); release_dev(h, s.d_tab); release_dev(h, s.d_w0); release_host(h, s.h_stage);
    const hipEvent_t ev = s.ev;
    s = ft8rx_handle::PreStream();
    s.ev = ev;
}

static int pre_stream_open(ft8rx_handle* h, const char* who, int which, int kind, int32_t rate_hz, int n_out, const double* f_dial_hz, float gain,
                           uint64_t n_origin, int keep_f32, double* f_mixed_hz) {
    if (!h) return -1;
    if (h->ps.open) {
        set_err(h, "%s: a %s stream is open on this handle%s (%s_stream_close)", who, h->ps.st.name, h->ps.st.which == which ? " already" : "", h->ps.st.entry);
        return -1;
    }
    if (h->ds.open) { set_err(h, "%s: a stream is open on this handle already (ft8rx_ddc_stream_close)", who); return -1; }
    PreStage d;
    if (pre_check(h, who, which, d, kind, rate_hz, n_out, f_dial_hz, gain) < 0) return -1;
    // the origin: k_origin = n_origin L / M lies on the tile grid of the stage behind (wide: n_origin is a multiple of 1008 rate / 12000)
    if (n_origin > (uint64_t)d.n_max || !ddcpre::origin_ok((int64_t)n_origin, d.n_max, d.rate_mid, d.L, d.M)) {
        if (which == PRE_WIDE)
            set_err(h, "%s: n_origin %llu is not a multiple of %llu (1008 rate_hz / 12000)", who, (unsigned long long)n_origin,
                    (unsigned long long)DDC_TO * ((unsigned long long)rate_hz / 12000));
        else
            set_err(h, "%s: n_origin %llu: n_origin L / M must be an integer multiple of %d (1008 rate_mid / 12000), n_origin <= 2^52", who,
                    (unsigned long long)n_origin, (int)(DDC_TO * (d.rate_mid / 12000)));
        return -1;
    }
    ENTER(h);
    PreTables t;
    pre_tables(d, n_out, f_dial_hz, t);
    std::vector<int32_t> src((size_t)n_out);
    for (int j = 0; j < n_out; j++) src[j] = j;
    // the stage behind: n_out IQ float32 streams at rate_mid, one channel each, from the same origin
    const int64_t k_origin = ddcpre::k_origin((int64_t)n_origin, d.L, d.M);
    if (const int rc = ddc_stream_open(h, FT8RX_DDC_IQ_F32, d.rate_mid, n_out, n_out, src.data(), t.dial_mid.data(), gain, (uint64_t)k_origin, keep_f32,
                                       f_mixed_hz)) return rc;
    ft8rx_handle::PreStream& s = h->ps;
    const int fmt = sample_fmt(kind);
    const size_t sb = sf_sample_bytes(fmt);
    int rc = 0;
    hipError_t e = hipSuccess;
    if (!s.ev) e = hipEventCreateWithFlags(&s.ev, hipEventDisableTiming);
    if (e != hipSuccess) { set_err(h, "%s: %s", who, hipGetErrorString(e)); rc = -2; }
    if (!rc) rc = dalloc(h, &s.d_hist, (size_t)d.H * sb);
    if (!rc) rc = dalloc(h, &s.d_chunk, (size_t)rate_hz * sb);
    if (!rc) rc = dalloc(h, &s.d_mid, (size_t)n_out * (size_t)d.rate_mid);
    if (!rc) rc = dalloc(h, &s.d_tab, t.tab.size());
    if (!rc) rc = dalloc(h, &s.d_w0, t.w0s.size());
    if (!rc) rc = halloc(h, &s.h_stage, (size_t)rate_hz * sb);
    if (!rc) {
        e = hipMemcpyAsync(s.d_tab, t.tab.data(), sizeof(float2) * t.tab.size(), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s.d_w0, t.w0s.data(), sizeof(uint32_t) * t.w0s.size(), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(s.d_hist, 0, (size_t)d.H * sb, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);      // the tables are pageable vectors of this call
        if (e != hipSuccess) { set_err(h, "%s: %s", who, hipGetErrorString(e)); rc = -2; }
    }
    if (rc) { pre_stream_release(h); ddc_stream_release(h); return -2; }
    pre_mixed(rate_hz, n_out, t.f0s, f_mixed_hz);
    s.st = d; s.fmt = fmt; s.n_out = n_out;
    s.n_origin = (int64_t)n_origin; s.pushed = 0; s.k_done = k_origin;
    s.open = true;
    return 0;
}

// the open stream of stage `which`, or nullptr with the error text
static ft8rx_handle::PreStream* pre_stream_of(ft8rx_handle* h, const char* who, int which, bool hint) {
    if (h->ps.open && h->ps.st.which == which) return &h->ps;
    if (hint) set_err(h, "%s: no %s stream is open (%s_stream_open)", who, PRE_NAME[which], PRE_ENTRY[which]);
    else set_err(h, "%s: no %s stream is open", who, PRE_NAME[which]);
    return nullptr;
}

static int pre_stream_push(ft8rx_handle* h, const char* who, int which, const void* in, uint64_t n_new, int on_device, uint64_t* m_produced) {
    if (!h) return -1;
    ft8rx_handle::PreStream* ps = pre_stream_of(h, who, which, true);
    if (!ps) return -1;
    ft8rx_handle::PreStream& s = *ps;
    const PreStage& d = s.st;
    if (n_new < 1 || n_new > (uint64_t)d.rate) { set_err(h, "%s: n_new %llu outside [1, %d] (one second)", who, (unsigned long long)n_new, (int)d.rate); return -1; }
    const size_t sb = sf_sample_bytes(s.fmt);
    if (!in || (on_device && ((uintptr_t)in % sb) != 0)) { set_err(h, "%s: in is NULL or not aligned to a sample", who); return -1; }
    if (s.n_origin + s.pushed + (int64_t)n_new > d.end_max) { set_err(h, "%s: n_new %llu takes the stream past index 2^53", who, (unsigned long long)n_new); return -1; }
    // (no ENTER: a push touches the streams' own buffers only, on the main stream; batches in flight read none of them)
    HIPCHK(h, hipSetDevice(h->device));
    const char* chunk = (const char*)in;
    if (!on_device) {                                    // through the page-locked buffer, once the previous push's copy has left it
        HIPCHK(h, hipEventSynchronize(s.ev));
        memcpy(s.h_stage, in, (size_t)n_new * sb);
        HIPCHK(h, hipMemcpyAsync(s.d_chunk, s.h_stage, (size_t)n_new * sb, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipEventRecord(s.ev, h->stream));
        chunk = s.d_chunk;
    }
    const int64_t n_start = s.n_origin + s.pushed, n_end = n_start + (int64_t)n_new;
    const int64_t k_new = ddcpre::mid_done(s.n_origin, n_end, d.n_taps, d.L, d.M);
    const int n_k = (int)(k_new - s.k_done);             // at most rate_mid: a push is at most a second
    if (n_k > 0) {
        pre_launch_stream(h, s, chunk, (long long)n_start, (long long)n_end, n_k);
        HIPCHK(h, hipGetLastError());
    }
    // the chunk's last H samples into the history, behind the kernel that read the old ones
    const ddcpre::Keep kp = ddcpre::keep(s.pushed, (int64_t)n_new, d.H);
    HIPCHK(h, hipMemcpyAsync(s.d_hist + (size_t)kp.pos * sb, chunk + (size_t)kp.skip * sb, (size_t)kp.first * sb, hipMemcpyDeviceToDevice, h->stream));
    if (kp.second) HIPCHK(h, hipMemcpyAsync(s.d_hist, chunk + (size_t)(kp.skip + kp.first) * sb, (size_t)kp.second * sb, hipMemcpyDeviceToDevice, h->stream));
    s.pushed += (int64_t)n_new;
    if (n_k > 0) {
        s.k_done = k_new;
        return ddc_stream_push(h, s.d_mid, (uint64_t)n_k, 1, m_produced);
    }
    if (m_produced) *m_produced = (uint64_t)(h->ds.tiles * DDC_TO);
    return 0;
}

static int pre_stream_read_mid(ft8rx_handle* h, const char* who, int which, uint64_t k_first_u, int n, float* mid) {
    if (!h) return -1;
    const ft8rx_handle::PreStream* ps = pre_stream_of(h, who, which, true);
    if (!ps) return -1;
    const ft8rx_handle::PreStream& s = *ps;
    const int64_t k_first = (int64_t)k_first_u, k_origin = ddcpre::k_origin(s.n_origin, s.st.L, s.st.M), cap = h->ds.cap;
    if (n < 1 || !mid || k_first < k_origin || k_first + n > s.k_done || k_first < s.k_done - cap) {
        set_err(h, "%s: intermediate samples [%lld, %lld) are not all held (held: %lld .. %lld)", who, (long long)k_first,
                (long long)(k_first + n), (long long)(s.k_done - cap > k_origin ? s.k_done - cap : k_origin), (long long)s.k_done);
        return -1;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // the stage behind keeps the newest `cap` samples of every channel: sample k at (k - k_origin) & (cap - 1)
    const int64_t pos = (k_first - k_origin) & (cap - 1), first = n < cap - pos ? n : cap - pos;
    const float2* ring = (const float2*)h->ds.d_in;
    float2* out = (float2*)mid;
    for (int j = 0; j < s.n_out; j++) {
        HIPCHK(h, hipMemcpy(out + (size_t)j * n, ring + (size_t)j * cap + pos, sizeof(float2) * (size_t)first, hipMemcpyDeviceToHost));
        if (first < n) HIPCHK(h, hipMemcpy(out + (size_t)j * n + first, ring + (size_t)j * cap, sizeof(float2) * (size_t)(n - first), hipMemcpyDeviceToHost));
    }
    return 0;
}

static int pre_stream_close(ft8rx_handle* h, const char* who, int which) {
    if (!h) return -1;
    if (!pre_stream_of(h, who, which, false)) return -1;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));          // pushes and gathers that still use the buffers
    pre_stream_release(h);
    ddc_stream_release(h);
    return 0;
}

int ft8rx_ddc_wide_stream_open(ft8rx_handle* h, int kind, int32_t rate_hz, int n_out, const double* f_dial_hz, float gain, uint64_t n_origin,
                               int keep_f32, double* f_mixed_hz) {
    return pre_stream_open(h, "ft8rx_ddc_wide_stream_open", PRE_WIDE, kind, rate_hz, n_out, f_dial_hz, gain, n_origin, keep_f32, f_mixed_hz);
}
int ft8rx_ddc_rat_stream_open(ft8rx_handle* h, int kind, int32_t rate_hz, int n_out, const double* f_dial_hz, float gain, uint64_t n_origin,
                              int keep_f32, double* f_mixed_hz) {
    return pre_stream_open(h, "ft8rx_ddc_rat_stream_open", PRE_RAT, kind, rate_hz, n_out, f_dial_hz, gain, n_origin, keep_f32, f_mixed_hz);
}
int ft8rx_ddc_wide_stream_push(ft8rx_handle* h, const void* in, uint64_t n_new, int on_device, uint64_t* m_produced) {
    return pre_stream_push(h, "ft8rx_ddc_wide_stream_push", PRE_WIDE, in, n_new, on_device, m_produced);
}
int ft8rx_ddc_rat_stream_push(ft8rx_handle* h, const void* in, uint64_t n_new, int on_device, uint64_t* m_produced) {
    return pre_stream_push(h, "ft8rx_ddc_rat_stream_push", PRE_RAT, in, n_new, on_device, m_produced);
}
int ft8rx_ddc_wide_stream_read_mid(ft8rx_handle* h, uint64_t k_first, int n, float* mid) {
    return pre_stream_read_mid(h, "ft8rx_ddc_wide_stream_read_mid", PRE_WIDE, k_first, n, mid);
}
int ft8rx_ddc_rat_stream_read_mid(ft8rx_handle* h, uint64_t k_first, int n, float* mid) {
    return pre_stream_read_mid(h, "ft8rx_ddc_rat_stream_read_mid", PRE_RAT, k_first, n, mid);
}
int ft8rx_ddc_wide_stream_close(ft8rx_handle* h) { return pre_stream_close(h, "ft8rx_ddc_wide_stream_close", PRE_WIDE); }
int ft8rx_ddc_rat_stream_close(ft8rx_handle* h) { return pre_stream_close(h, "ft8rx_ddc_rat_stream_close", PRE_RAT); }

// ---- noise blanker (kernels/blanker.hpp)
// T[1 .. R] of taper = R at t[1 .. R] (t[0] is not used): computed in double, rounded once
static void blank_taper(int R, int32_t* t) {
    t[0] = 0;
    for (int j = 1; j <= R; j++) t[j] = (int32_t)nearbyint(32768.0 * 0.5 * (1.0 - cos(M_PI * (double)j / (double)(R + 1))));
}

int ft8rx_blank_taper(int taper, int32_t* w, int cap) {
    if (taper < 0 || taper > FT8RX_BLANK_MAX_TAPER) return -1;
    int32_t t[FT8RX_BLANK_MAX_TAPER + 1];
    blank_taper(taper, t);
    for (int j = 1; w && j <= taper && j <= cap; j++) w[j - 1] = t[j];
    return taper;
}

static int blank_workspaces(ft8rx_handle* h) {
    if (ws_ready(h, WS_BLANK)) return 0;
    static_assert(BLK_TAPER_ROW == FT8RX_BLANK_MAX_TAPER + 1 && BLK_HALO == FT8RX_BLANK_MAX_GUARD + FT8RX_BLANK_MAX_TAPER &&
                  BLK_N * BLK_PER_FRAME == FT8RX_NSAMP && 8 * BLK_GROUPS == FT8RX_NSAMP && 64 * BLK_WORDS >= FT8RX_NSAMP &&
                  BLK_TILES * BLK_NT >= BLK_GROUPS && BLK_TILES * 32 >= BLK_WORDS, "blanker geometry");
    std::vector<int32_t> tab((size_t)BLK_TAPER_ROW * BLK_TAPER_ROW, 0);
    for (int R = 0; R <= FT8RX_BLANK_MAX_TAPER; R++) blank_taper(R, &tab[(size_t)R * BLK_TAPER_ROW]);
    FirstUse F(h, WS_BLANK);
    F.dev(&h->d_bl_lv, (size_t)h->max_frames * BLK_PER_FRAME * 2);
    F.dev(&h->d_bl_mask, (size_t)h->max_frames * BLK_WORDS);
    F.dev(&h->d_bl_part, (size_t)h->max_frames * BLK_TILES * 4);
    F.dev(&h->d_bl_stats, (size_t)h->max_frames * 4);
    F.dev(&h->d_bl_taper, tab.size());
    // (the upper half of a frame's last mask word is never written: it stays zero from here on)
    FIRST_HIP(F, hipMemset(h->d_bl_mask, 0, sizeof(uint64_t) * (size_t)h->max_frames * BLK_WORDS));
    FIRST_HIP(F, hipMemcpy(h->d_bl_taper, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice));
    return F.done();
}

static int blank_check(ft8rx_handle* h, const char* who, int n_frames, int32_t threshold_q8, int guard, int taper) {
    if (n_frames < 1 || n_frames > h->max_frames) { set_err(h, "%s: n_frames %d outside [1, %d] (max_frames)", who, n_frames, h->max_frames); return -1; }
    if (threshold_q8 < FT8RX_BLANK_MIN_THRESHOLD_Q8 || threshold_q8 > FT8RX_BLANK_MAX_THRESHOLD_Q8) {
        set_err(h, "%s: threshold_q8 %d outside [%d, %d] (256 k, k = 2 .. 64)", who, (int)threshold_q8, FT8RX_BLANK_MIN_THRESHOLD_Q8, FT8RX_BLANK_MAX_THRESHOLD_Q8); return -1;
    }
    if (guard < 0 || guard > FT8RX_BLANK_MAX_GUARD) { set_err(h, "%s: guard %d outside [0, %d]", who, guard, FT8RX_BLANK_MAX_GUARD); return -1; }
    if (taper < 0 || taper > FT8RX_BLANK_MAX_TAPER) { set_err(h, "%s: taper %d outside [0, %d]", who, taper, FT8RX_BLANK_MAX_TAPER); return -1; }
    return 0;
}

// the launches on the main stream, then -- stats or levels given -- their copies and the wait for them
static int blank_run(ft8rx_handle* h, int16_t* d_audio, int n_frames, int32_t threshold_q8, int guard, int taper, int32_t* stats, int32_t* levels) {
    const int n_blocks = n_frames * BLK_PER_FRAME;
    const dim3 tiles(BLK_TILES, (unsigned)n_frames);
    with_bool(((uintptr_t)d_audio % 16) == 0, [&](auto vec) {
        constexpr bool V = decltype(vec)::value;
        k_blank_level<V><<<(n_blocks + BLK_NT / 64 - 1) / (BLK_NT / 64), BLK_NT, 0, h->stream>>>(d_audio, n_blocks, h->d_bl_lv);
        k_blank_hits<V><<<tiles, BLK_NT, 0, h->stream>>>(d_audio, threshold_q8, h->d_bl_lv, reinterpret_cast<uint8_t*>(h->d_bl_mask), h->d_bl_part);
        k_blank_gate<V><<<tiles, BLK_NT, 0, h->stream>>>(d_audio, h->d_bl_mask, guard, taper, h->d_bl_taper, h->d_bl_part);
    });
    if (stats) k_blank_stats<<<(4 * n_frames + BLK_NT - 1) / BLK_NT, BLK_NT, 0, h->stream>>>(h->d_bl_part, n_frames, h->d_bl_stats);
    HIPCHK(h, hipGetLastError());
    if (stats) HIPCHK(h, hipMemcpyAsync(stats, h->d_bl_stats, sizeof(int32_t) * 4 * (size_t)n_frames, hipMemcpyDeviceToHost, h->stream));
    if (levels) HIPCHK(h, hipMemcpyAsync(levels, h->d_bl_lv, sizeof(int32_t) * 2 * (size_t)n_blocks, hipMemcpyDeviceToHost, h->stream));
    if (stats || levels) HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int ft8rx_blank(ft8rx_handle* h, int16_t* d_audio, int n_frames, int32_t threshold_q8, int guard, int taper, int32_t* stats, int32_t* levels) {
    if (!h) return -1;
    if (blank_check(h, "ft8rx_blank", n_frames, threshold_q8, guard, taper)) return -1;
    if (((uintptr_t)d_audio % sizeof(int16_t)) != 0) { set_err(h, "ft8rx_blank: d_audio is not aligned to a sample"); return -1; }
    ENTER(h);
    if (blank_workspaces(h)) return -2;
    if (!d_audio) { if (need_staging(h)) return -2; d_audio = h->d_audio; }
    return blank_run(h, d_audio, n_frames, threshold_q8, guard, taper, stats, levels);
}

int ft8rx_blank_host(ft8rx_handle* h, const int16_t* audio, int n_frames, int32_t threshold_q8, int guard, int taper, int32_t* stats) {
    if (!h) return -1;
    if (blank_check(h, "ft8rx_blank_host", n_frames, threshold_q8, guard, taper)) return -1;
    if (!audio) { set_err(h, "ft8rx_blank_host: audio is NULL"); return -1; }
    ENTER(h);
    if (blank_workspaces(h) || need_staging(h)) return -2;
    HIPCHK(h, hipMemcpyAsync(h->d_audio, audio, sizeof(int16_t) * (size_t)n_frames * FT8RX_NSAMP, hipMemcpyHostToDevice, h->stream));
    if (const int rc = blank_run(h, h->d_audio, n_frames, threshold_q8, guard, taper, stats, nullptr)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// ---- input-rate noise blanker (kernels/blank_in.hpp; the index arithmetic is blank_in_ring.hpp's)
static int blank_in_log2(int block) {
    for (int k = 8; k <= 12; k++) if (block == (1 << k)) return k;
    return -1;
}
// the text of a refusal -> err (host only: ft8rx_blank_in_released has no handle), or nullptr
static const char* blank_in_refusal(int kind, bool with_kind, int block, int32_t threshold_q8, int guard, int taper, char* err, size_t cap) {
    static_assert(FT8RX_BLANK_IN_MIN_BLOCK == 256 && FT8RX_BLANK_IN_MAX_BLOCK == 4096 && BIN_HALO == FT8RX_BLANK_MAX_GUARD + FT8RX_BLANK_MAX_TAPER &&
                  BIN_TAPER_ROW == FT8RX_BLANK_MAX_TAPER + 1 && FT8RX_BLANK_IN_MAX_BLOCK <= 16 * BIN_NT, "input blanker geometry");
    if (with_kind && !sf_kind_in(SF_KINDS_BLANK_IN, kind)) snprintf(err, cap, "kind %d is not an integer kind (real int16, IQ int16, IQ uint8, IQ int8)", kind);
    else if (blank_in_log2(block) < 0) snprintf(err, cap, "block %d is not a power of two in [%d, %d]", block, FT8RX_BLANK_IN_MIN_BLOCK, FT8RX_BLANK_IN_MAX_BLOCK);
    else if (threshold_q8 < FT8RX_BLANK_MIN_THRESHOLD_Q8 || threshold_q8 > FT8RX_BLANK_MAX_THRESHOLD_Q8)
        snprintf(err, cap, "threshold_q8 %d outside [%d, %d] (256 k, k = 2 .. 64)", (int)threshold_q8, FT8RX_BLANK_MIN_THRESHOLD_Q8, FT8RX_BLANK_MAX_THRESHOLD_Q8);
    else if (guard < 0 || guard > FT8RX_BLANK_MAX_GUARD) snprintf(err, cap, "guard %d outside [0, %d]", guard, FT8RX_BLANK_MAX_GUARD);
    else if (taper < 0 || taper > FT8RX_BLANK_MAX_TAPER) snprintf(err, cap, "taper %d outside [0, %d]", taper, FT8RX_BLANK_MAX_TAPER);
    else return nullptr;
    return err;
}
// the argument checks of an entry -> the format of its kind, or -1 with the error text
static int blank_in_check(ft8rx_handle* h, const char* who, int kind, int block, int32_t threshold_q8, int guard, int taper) {
    char text[200];
    if (!blank_in_refusal(kind, true, block, threshold_q8, guard, taper, text, sizeof(text))) return sample_fmt(kind);
    set_err(h, "%s: %s", who, text);
    return -1;
}

int ft8rx_blank_in_released(uint64_t n_origin, uint64_t n_end, int block, int guard, int taper, uint64_t* released) {
    char text[200];
    if (blank_in_refusal(0, false, block, FT8RX_BLANK_IN_THRESHOLD_Q8_DEFAULT_REAL, guard, taper, text, sizeof(text))) return -1;
    if (n_end < n_origin || n_end > ((uint64_t)1 << 62)) return -1;
    if (released) *released = (uint64_t)blankin::released((int64_t)n_origin, (int64_t)n_end, block, guard, taper);
    return 0;
}

// the taper tables (shared by the one-shot entries and the stream; 17 KB, made once)
static int blank_in_tables(ft8rx_handle* h) {
    if (ws_ready(h, WS_BLANK_IN)) return 0;
    std::vector<int32_t> tab((size_t)BIN_TAPER_ROW * BIN_TAPER_ROW, 0);
    for (int R = 0; R <= FT8RX_BLANK_MAX_TAPER; R++) blank_taper(R, &tab[(size_t)R * BIN_TAPER_ROW]);
    FirstUse F(h, WS_BLANK_IN);
    F.dev(&h->d_bi_taper, tab.size());
    FIRST_HIP(F, hipMemcpy(h->d_bi_taper, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice));
    return F.done();
}

// what a run of at most n_max new samples needs: every ring holds what a push reads of the pushes before it (blank_in_ring.hpp)
struct BlankInSizes { size_t lv_cap, mask_words, part_cap; };
static BlankInSizes blank_in_sizes(int64_t n_max, int64_t B) {
    BlankInSizes z{16, 64, 0};
    while ((int64_t)z.lv_cap < n_max / B + 16) z.lv_cap *= 2;
    while ((int64_t)z.mask_words * 64 < n_max + 8 * B + 8192) z.mask_words *= 2;
    z.part_cap = (size_t)((n_max + 8 * B + 256) / 2048 + 4);
    return z;
}
static void blank_in_ws_release(ft8rx_handle* h, ft8rx_handle::BlankInWs& w) {
    release_dev(h, w.d_lv); release_dev(h, w.d_mask); release_dev(h, w.d_part_h); release_dev(h, w.d_part_g); release_dev(h, w.d_stats);
    w = ft8rx_handle::BlankInWs();
}
// all or nothing; a workspace that is large enough stays
static int blank_in_ws_alloc(ft8rx_handle* h, ft8rx_handle::BlankInWs& w, const BlankInSizes& z) {
    if (w.d_lv && w.lv_cap >= z.lv_cap && w.mask_words >= z.mask_words && w.part_cap >= z.part_cap) return 0;
    blank_in_ws_release(h, w);
    int rc = dalloc(h, &w.d_lv, 2 * z.lv_cap);
    if (!rc) rc = dalloc(h, &w.d_mask, z.mask_words);
    if (!rc) rc = dalloc(h, &w.d_part_h, 2 * z.part_cap);
    if (!rc) rc = dalloc(h, &w.d_part_g, 2 * z.part_cap);
    if (!rc) rc = dalloc(h, &w.d_stats, (size_t)4);
    if (rc) { blank_in_ws_release(h, w); return -2; }
    w.lv_cap = z.lv_cap; w.mask_words = z.mask_words; w.part_cap = z.part_cap;
    return 0;
}

// The launches of one plan on the main stream.  x: the sample of absolute index p.base; the stream's samples [n_origin, p.n_end) exist.
static int blank_in_launch(ft8rx_handle* h, ft8rx_handle::BlankInWs& w, int fmt, char* x, const blankin::Plan& p, int64_t n_origin, int log2_b,
                           int32_t threshold_q8, int guard, int taper) {
    const int64_t B = (int64_t)1 << log2_b;
    const BinWin W{x, (long long)p.base, (long long)n_origin, (long long)p.n_end};
    const int64_t n_lv = p.lv1 - p.lv0, n_h = ((p.hb1 - p.hb0) * (B / 8) + BIN_NT - 1) / BIN_NT;
    const int64_t n_g = p.g1 > p.g0 ? ((p.g1 - 1) >> 11) - (p.g0 >> 11) + 1 : 0;
    if (n_h > (int64_t)w.part_cap || n_g > (int64_t)w.part_cap || n_lv + 8 > (int64_t)w.lv_cap) { set_err(h, "input blanker: a plan beyond its workspaces"); return -2; }
    const bool vec = ((uintptr_t)x % 16) == 0;
    auto run = [&](auto f, auto v) {
        constexpr int F = decltype(f)::value;
        constexpr bool V = decltype(v)::value;
        if (n_lv > 0) k_blankin_level<F, V><<<(unsigned)n_lv, BIN_NT, 0, h->stream>>>(W, log2_b, (long long)p.lv0, w.d_lv, (int)w.lv_cap);
        if (n_h > 0)
            k_blankin_hits<F, V><<<(unsigned)n_h, BIN_NT, 0, h->stream>>>(W, log2_b, (long long)p.hb0, (long long)p.hb1, (long long)p.b_first, (long long)p.b_have,
                                                                       (long long)(p.n_end / B), threshold_q8, w.d_lv, (int)w.lv_cap,
                                                                       reinterpret_cast<uint8_t*>(w.d_mask), (long long)(8 * w.mask_words), w.d_part_h);
        if (n_g > 0)
            k_blankin_gate<F, V><<<(unsigned)n_g, BIN_NT, 0, h->stream>>>(W, (long long)p.g0, (long long)p.g1, (long long)(p.b_first * B), (long long)p.m_hi, w.d_mask,
                                                                       (long long)w.mask_words, guard, taper, h->d_bi_taper, w.d_part_g);
    };
    with_bool(vec, [&](auto v) {
        switch (fmt) {
            case SF_REAL_I16: run(std::integral_constant<int, SF_REAL_I16>(), v); break;
            case SF_IQ_I16: run(std::integral_constant<int, SF_IQ_I16>(), v); break;
            case SF_IQ_U8: run(std::integral_constant<int, SF_IQ_U8>(), v); break;
            default: run(std::integral_constant<int, SF_IQ_I8>(), v); break;
        }
    });
    if (n_h > 0 || n_g > 0) k_blankin_stats<<<1, BIN_NT, 0, h->stream>>>(w.d_part_h, (int)n_h, w.d_part_g, (int)n_g, w.d_stats);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// the one-shot on n samples at d: the stream with n_origin = 0, pushed n samples and finished
static int blank_in_oneshot(ft8rx_handle* h, char* d, int fmt, uint64_t n_samples, int block, int32_t threshold_q8, int guard, int taper, int64_t* stats,
                            int32_t* levels) {
    const int log2_b = blank_in_log2(block);
    if (blank_in_tables(h) || blank_in_ws_alloc(h, h->bi, blank_in_sizes((int64_t)n_samples, block))) return -2;
    const blankin::Plan p = blankin::plan(0, 0, (int64_t)n_samples, true, block, guard, taper);
    HIPCHK(h, hipMemsetAsync(h->bi.d_stats, 0, sizeof(long long) * 4, h->stream));
    if (const int rc = blank_in_launch(h, h->bi, fmt, d, p, 0, log2_b, threshold_q8, guard, taper)) return rc;
    if (stats) HIPCHK(h, hipMemcpyAsync(stats, h->bi.d_stats, sizeof(int64_t) * 4, hipMemcpyDeviceToHost, h->stream));
    if (levels) HIPCHK(h, hipMemcpyAsync(levels, h->bi.d_lv, sizeof(int32_t) * 2 * (size_t)p.b_have, hipMemcpyDeviceToHost, h->stream));
    if (stats || levels) HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}
static int blank_in_n_check(ft8rx_handle* h, const char* who, uint64_t n_samples) {
    if (n_samples >= 1 && n_samples <= FT8RX_BLANK_IN_MAX_SAMPLES) return 0;
    set_err(h, "%s: n_samples %llu outside [1, %llu]", who, (unsigned long long)n_samples, (unsigned long long)FT8RX_BLANK_IN_MAX_SAMPLES);
    return -1;
}

int ft8rx_blank_in(ft8rx_handle* h, void* d_samples, int kind, uint64_t n_samples, int block, int32_t threshold_q8, int guard, int taper, void* d_out,
                   int64_t* stats, int32_t* levels) {
    if (!h) return -1;
    const int fmt = blank_in_check(h, "ft8rx_blank_in", kind, block, threshold_q8, guard, taper);
    if (fmt < 0 || blank_in_n_check(h, "ft8rx_blank_in", n_samples)) return -1;
    const size_t sb = sf_sample_bytes(fmt), align = sf_component_bytes(fmt);      // (the messages' "sample": a component is enough)
    if (!d_samples || ((uintptr_t)d_samples % align) != 0) { set_err(h, "ft8rx_blank_in: d_samples is NULL or not aligned to a sample"); return -1; }
    if (((uintptr_t)d_out % align) != 0) { set_err(h, "ft8rx_blank_in: d_out is not aligned to a sample"); return -1; }
    ENTER(h);
    if (d_out && d_out != d_samples) HIPCHK(h, hipMemcpyAsync(d_out, d_samples, (size_t)n_samples * sb, hipMemcpyDeviceToDevice, h->stream));
    return blank_in_oneshot(h, (char*)(d_out ? d_out : d_samples), fmt, n_samples, block, threshold_q8, guard, taper, stats, levels);
}

int ft8rx_blank_in_host(ft8rx_handle* h, const void* samples, int kind, uint64_t n_samples, int block, int32_t threshold_q8, int guard, int taper,
                        int64_t* stats, void** d_out) {
    if (!h) return -1;
    const int fmt = blank_in_check(h, "ft8rx_blank_in_host", kind, block, threshold_q8, guard, taper);
    if (fmt < 0 || blank_in_n_check(h, "ft8rx_blank_in_host", n_samples)) return -1;
    if (!samples) { set_err(h, "ft8rx_blank_in_host: samples is NULL"); return -1; }
    const size_t bytes = (size_t)n_samples * sf_sample_bytes(fmt);
    ENTER(h);
    if (h->bi_buf_cap < bytes) {
        HIPCHK(h, hipStreamSynchronize(h->stream));     // what was queued behind the last call still reads the old buffer
        release_dev(h, h->d_bi_buf); h->d_bi_buf = nullptr; h->bi_buf_cap = 0;
        if (dalloc(h, &h->d_bi_buf, bytes)) return -2;
        h->bi_buf_cap = bytes;
    }
    HIPCHK(h, hipMemcpyAsync(h->d_bi_buf, samples, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));         // the caller's memory is free again
    if (const int rc = blank_in_oneshot(h, h->d_bi_buf, fmt, n_samples, block, threshold_q8, guard, taper, stats, nullptr)) return rc;
    if (d_out) *d_out = h->d_bi_buf;
    return 0;
}

static void blank_in_stream_release(ft8rx_handle* h) {
    ft8rx_handle::BlankInStream& s = h->bis;
    release_dev(h, s.d_work[0]); release_dev(h, s.d_work[1]); release_host(h, s.h_stage);
    blank_in_ws_release(h, s.ws);
    const hipEvent_t ev = s.ev;
    s = ft8rx_handle::BlankInStream();
    s.ev = ev;
}

int ft8rx_blank_in_stream_open(ft8rx_handle* h, int kind, int block, int32_t threshold_q8, int guard, int taper, uint64_t n_origin, uint64_t max_push) {
    if (!h) return -1;
    const char* who = "ft8rx_blank_in_stream_open";
    if (h->bis.open) { set_err(h, "%s: an input blanker stream is open on this handle already (ft8rx_blank_in_stream_close)", who); return -1; }
    const int fmt = blank_in_check(h, who, kind, block, threshold_q8, guard, taper);
    if (fmt < 0) return -1;
    if (n_origin > ((uint64_t)1 << 53)) { set_err(h, "%s: n_origin %llu beyond 2^53", who, (unsigned long long)n_origin); return -1; }
    if (max_push < 1 || max_push > FT8RX_BLANK_IN_MAX_PUSH) {
        set_err(h, "%s: max_push %llu outside [1, %llu]", who, (unsigned long long)max_push, (unsigned long long)FT8RX_BLANK_IN_MAX_PUSH); return -1;
    }
    ENTER(h);
    if (blank_in_tables(h)) return -2;
    ft8rx_handle::BlankInStream& s = h->bis;
    const size_t sb = sf_sample_bytes(fmt), work = (size_t)blankin::capacity(block, guard, taper, (int64_t)max_push) * sb;
    int rc = 0;
    hipError_t e = hipSuccess;
    if (!s.ev) e = hipEventCreateWithFlags(&s.ev, hipEventDisableTiming);
    if (e != hipSuccess) { set_err(h, "%s: %s", who, hipGetErrorString(e)); rc = -2; }
    if (!rc) rc = dalloc(h, &s.d_work[0], work);
    if (!rc) rc = dalloc(h, &s.d_work[1], work);
    if (!rc) rc = halloc(h, &s.h_stage, (size_t)max_push * sb);
    if (!rc) rc = blank_in_ws_alloc(h, s.ws, blank_in_sizes((int64_t)max_push, block));
    if (!rc && (e = hipMemsetAsync(s.ws.d_stats, 0, sizeof(long long) * 4, h->stream)) != hipSuccess) { set_err(h, "%s: %s", who, hipGetErrorString(e)); rc = -2; }
    if (rc) { blank_in_stream_release(h); return -2; }
    s.fmt = fmt; s.log2_b = blank_in_log2(block); s.threshold_q8 = threshold_q8; s.guard = guard; s.taper = taper;
    s.n_origin = (int64_t)n_origin; s.pushed = 0; s.max_push = (int64_t)max_push; s.base = (int64_t)n_origin / block * block; s.cur = 0;
    s.finished = false; s.open = true;
    return 0;
}

int ft8rx_blank_in_stream_push(ft8rx_handle* h, const void* in, uint64_t n_new, int on_device, int finish, void** d_out, uint64_t* n_first,
                               uint64_t* n_out) {
    if (!h) return -1;
    const char* who = "ft8rx_blank_in_stream_push";
    ft8rx_handle::BlankInStream& s = h->bis;
    if (!s.open) { set_err(h, "%s: no input blanker stream is open (ft8rx_blank_in_stream_open)", who); return -1; }
    if (s.finished) { set_err(h, "%s: the stream is finished: only ft8rx_blank_in_stream_info and ft8rx_blank_in_stream_close are accepted", who); return -1; }
    if (n_new > (uint64_t)s.max_push) { set_err(h, "%s: n_new %llu outside [0, %llu] (max_push)", who, (unsigned long long)n_new, (unsigned long long)s.max_push); return -1; }
    const size_t sb = sf_sample_bytes(s.fmt), align = sf_component_bytes(s.fmt);
    if (n_new && (!in || (on_device && ((uintptr_t)in % align) != 0))) { set_err(h, "%s: in is NULL or not aligned to a sample", who); return -1; }
    if (s.n_origin + s.pushed + (int64_t)n_new > ((int64_t)1 << 54)) { set_err(h, "%s: n_new %llu takes the stream past index 2^54", who, (unsigned long long)n_new); return -1; }
    // (no ENTER: a push touches the stream's own buffers only, on the main stream; batches in flight read none of them)
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t B = (int64_t)1 << s.log2_b, n_start = s.n_origin + s.pushed;
    const blankin::Plan p = blankin::plan(s.n_origin, n_start, (int64_t)n_new, finish != 0, B, s.guard, s.taper);
    // the other work buffer: the leftover to its front -- behind whatever consumed the samples the last push released -- then the chunk
    char* old = s.d_work[s.cur];
    char* x = s.d_work[s.cur ^ 1];
    if (p.left_n > 0)
        HIPCHK(h, hipMemcpyAsync(x + (size_t)(p.g0 - p.base) * sb, old + (size_t)(p.g0 - s.base) * sb, (size_t)p.left_n * sb, hipMemcpyDeviceToDevice, h->stream));
    if (n_new) {
        char* dst = x + (size_t)(n_start - p.base) * sb;
        if (on_device) {
            HIPCHK(h, hipMemcpyAsync(dst, in, (size_t)n_new * sb, hipMemcpyDeviceToDevice, h->stream));
        } else {                                         // through the page-locked buffer, once the previous push's copy has left it
            HIPCHK(h, hipEventSynchronize(s.ev));
            memcpy(s.h_stage, in, (size_t)n_new * sb);
            HIPCHK(h, hipMemcpyAsync(dst, s.h_stage, (size_t)n_new * sb, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipEventRecord(s.ev, h->stream));
        }
    }
    if (const int rc = blank_in_launch(h, s.ws, s.fmt, x, p, s.n_origin, s.log2_b, s.threshold_q8, s.guard, s.taper)) return rc;
    s.cur ^= 1; s.base = p.base; s.pushed += (int64_t)n_new; s.finished = finish != 0;
    if (d_out) *d_out = x + (size_t)(p.g0 - p.base) * sb;
    if (n_first) *n_first = (uint64_t)p.g0;
    if (n_out) *n_out = (uint64_t)(p.g1 - p.g0);
    return 0;
}

int ft8rx_blank_in_stream_info(ft8rx_handle* h, uint64_t* n_pushed, uint64_t* n_released, int64_t* stats) {
    if (!h) return -1;
    const ft8rx_handle::BlankInStream& s = h->bis;
    if (!s.open) { set_err(h, "ft8rx_blank_in_stream_info: no input blanker stream is open (ft8rx_blank_in_stream_open)"); return -1; }
    const int64_t n_end = s.n_origin + s.pushed;
    if (n_pushed) *n_pushed = (uint64_t)s.pushed;
    if (n_released) *n_released = (uint64_t)(s.finished ? n_end : blankin::released(s.n_origin, n_end, (int64_t)1 << s.log2_b, s.guard, s.taper));
    if (stats) {
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipMemcpyAsync(stats, s.ws.d_stats, sizeof(int64_t) * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return 0;
}

int ft8rx_blank_in_stream_close(ft8rx_handle* h) {
    if (!h) return -1;
    if (!h->bis.open) { set_err(h, "ft8rx_blank_in_stream_close: no input blanker stream is open"); return -1; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));          // pushes, and what consumed the released samples
    blank_in_stream_release(h);
    return 0;
}

// ---- panorama (kernels/pan.hpp; the index arithmetic is pan_ring.hpp's)
#define PAN_TILE_BYTES ((size_t)32 << 20)      /* the powers of one tile of windows: what k_pan_power writes and k_pan_rows reads back */
static_assert(FT8RX_PAN_MIN_FFT == 256 && FT8RX_PAN_MAX_FFT == PAN_TW_N && FT8RX_PAN_MIN_FFT / 2 % PAN_ROWS_NT == 0 && PAN_ROWS_NT == 128 &&
              (uint64_t)FT8RX_PAN_MAX_FFT * FT8RX_PAN_MAX_AVG <= (1ull << 29), "panorama geometry: bins in 128s, a row's count in int32");
// the text of a refusal -> err (host only: ft8rx_pan_rows_done has no handle), or nullptr
static const char* pan_refusal(int kind, bool with_kind, int n_fft, int n_avg, char* err, size_t cap) {
    if (with_kind && sample_fmt(kind) < 0) snprintf(err, cap, "kind %d is none of the sample kinds (FT8RX_DDC_*, FT8RX_WIDE_*)", kind);
    else if (n_fft < FT8RX_PAN_MIN_FFT || n_fft > FT8RX_PAN_MAX_FFT || (n_fft & (n_fft - 1)))
        snprintf(err, cap, "n_fft %d is not a power of two in [%d, %d]", n_fft, FT8RX_PAN_MIN_FFT, FT8RX_PAN_MAX_FFT);
    else if (n_avg < 1 || n_avg > FT8RX_PAN_MAX_AVG) snprintf(err, cap, "n_avg %d outside [1, %d]", n_avg, FT8RX_PAN_MAX_AVG);
    else return nullptr;
    return err;
}
static int pan_check(ft8rx_handle* h, const char* who, int kind, int n_fft, int n_avg) {
    char text[200];
    if (!pan_refusal(kind, true, n_fft, n_avg, text, sizeof(text))) return sample_fmt(kind);
    set_err(h, "%s: %s", who, text);
    return -1;
}

// the periodic Hann window, in double, rounded once
static void pan_window(int N, float* w) {
    for (int i = 0; i < N; i++) w[i] = (float)(0.5 * (1.0 - cos(2.0 * M_PI * (double)i / (double)N)));
}
int ft8rx_pan_window(int n_fft, float* w, int cap) {
    char text[200];
    if (pan_refusal(0, false, n_fft, 1, text, sizeof(text))) return -1;
    if (w && cap > 0) {
        std::vector<float> t((size_t)n_fft);
        pan_window(n_fft, t.data());
        memcpy(w, t.data(), sizeof(float) * (size_t)(cap < n_fft ? cap : n_fft));
    }
    return n_fft;
}
int ft8rx_pan_rows_done(uint64_t n_origin, uint64_t n_end, int n_fft, int n_avg, uint64_t* rows) {
    char text[200];
    if (pan_refusal(0, false, n_fft, n_avg, text, sizeof(text))) return -1;
    if (n_end < n_origin || n_end > ((uint64_t)1 << 62)) return -1;
    if (rows) {
        rows[0] = (uint64_t)panring::r_first((int64_t)n_origin, n_fft, n_avg);
        rows[1] = (uint64_t)panring::rows_done((int64_t)n_origin, (int64_t)n_end, n_fft, n_avg);
    }
    return 0;
}

// the twiddles W_8192^k: the quarter turn in double, the quadrants by exact rotation, rounded once; and the one-shot entries' weight table
static int pan_tables(ft8rx_handle* h) {
    if (ws_ready(h, WS_PAN)) return 0;
    std::vector<cpx> tw((size_t)PAN_TW_N);
    for (int k = 0; k < PAN_TW_N; k++) {
        const int q = k / (PAN_TW_N / 4), r = k % (PAN_TW_N / 4);
        const double c = r ? cos(2.0 * M_PI * r / PAN_TW_N) : 1.0, s = r ? sin(2.0 * M_PI * r / PAN_TW_N) : 0.0;      // e^(-i a) = (c, -s)
        const double re[4] = {c, -s, -c, s}, im[4] = {-s, -c, s, c};                                           // times (-i)^q
        tw[(size_t)k] = make_float2((float)re[q], (float)im[q]);
    }
    FirstUse F(h, WS_PAN);
    F.dev(&h->d_pan_tw, tw.size());
    F.dev(&h->pan.d_win, (size_t)PAN_TW_N);
    FIRST_HIP(F, hipMemcpy(h->d_pan_tw, tw.data(), sizeof(cpx) * tw.size(), hipMemcpyHostToDevice));
    return F.done();
}
// windows per tile of a workspace for `bins` bins that never sees more than max_win windows in one run
static size_t pan_tile_cap(int bins, int64_t max_win) {
    const size_t t = PAN_TILE_BYTES / (sizeof(float) * (size_t)bins);
    return (int64_t)t < max_win ? t : (size_t)(max_win > 1 ? max_win : 1);
}

// The launches of the windows [w0, w0 + n_win) on the main stream: x = the first sample of window w0.
static int pan_run(ft8rx_handle* h, const ft8rx_handle::PanWs& w, int fmt, int N, int A, const char* x, int64_t w0, int64_t n_win) {
    const bool iq = sf_is_iq(fmt), aligned = ((uintptr_t)x % sf_sample_bytes(fmt)) == 0;
    const int bins = iq ? N : N / 2;
    const size_t sb = sf_sample_bytes(fmt);
    for (int64_t t = 0; t < n_win; t += (int64_t)w.tile_w) {
        const int64_t nw = n_win - t < (int64_t)w.tile_w ? n_win - t : (int64_t)w.tile_w, wa = w0 + t;
        const char* xt = x + (size_t)t * (size_t)N * sb;
        auto power = [&](auto n, auto q, auto al) {
            constexpr int NN = decltype(n)::value;
            k_pan_power<NN, decltype(q)::value, decltype(al)::value><<<(unsigned)nw, pan_nt(NN), 0, h->stream>>>(xt, fmt, w.d_win, h->d_pan_tw, w.d_pw, w.d_wstat);
        };
        with_bool(iq, [&](auto q) { with_bool(aligned, [&](auto al) {
            switch (N) {
                case 256: power(std::integral_constant<int, 256>(), q, al); break;
                case 512: power(std::integral_constant<int, 512>(), q, al); break;
                case 1024: power(std::integral_constant<int, 1024>(), q, al); break;
                case 2048: power(std::integral_constant<int, 2048>(), q, al); break;
                case 4096: power(std::integral_constant<int, 4096>(), q, al); break;
                default: power(std::integral_constant<int, 8192>(), q, al); break;
            }
        }); });
        const int64_t ra = wa / A, rb = (wa + nw - 1) / A;
        k_pan_rows<<<dim3((unsigned)(rb - ra + 1), (unsigned)(bins / PAN_ROWS_NT + 1)), PAN_ROWS_NT, 0, h->stream>>>(
            w.d_pw, w.d_wstat, (long long)wa, (int)nw, (long long)A, bins, (long long)ra, w.d_ring, w.d_rstat, (long long)w.slots);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

// the one-shot on n samples at d: the stream with n_origin = 0 and a ring that holds every row
static int pan_oneshot(ft8rx_handle* h, const char* who, const char* d, int fmt, uint64_t n_samples, int N, int A, float* rows, int32_t* stats, uint64_t* n_rows_out) {
    const int64_t R = (int64_t)(n_samples / (uint64_t)N) / A;
    if (n_rows_out) *n_rows_out = (uint64_t)R;
    if (R == 0 || (!rows && !stats)) return 0;
    const int bins = sf_is_iq(fmt) ? N : N / 2;
    if (pan_tables(h)) return -2;
    ft8rx_handle::PanWs& w = h->pan;
    const size_t tile = pan_tile_cap(bins, R * A);
    if (grow_dev(h, who, (void**)&w.d_pw, &h->pan_pw_cap, sizeof(float) * tile * (size_t)bins) ||
        grow_dev(h, who, (void**)&w.d_wstat, &h->pan_wstat_cap, sizeof(int32_t) * 2 * tile) ||
        grow_dev(h, who, (void**)&w.d_ring, &h->pan_ring_cap, sizeof(float) * (size_t)R * (size_t)bins) ||
        grow_dev(h, who, (void**)&w.d_rstat, &h->pan_rstat_cap, sizeof(int32_t) * 2 * (size_t)R)) return -2;
    w.tile_w = tile; w.slots = (size_t)R;
    if (w.win_n != N) {                                   // another n_fft than the last call's: nothing queued reads the old table any more
        std::vector<float> t((size_t)N);
        pan_window(N, t.data());
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(w.d_win, t.data(), sizeof(float) * (size_t)N, hipMemcpyHostToDevice));
        w.win_n = N;
    }
    if (const int rc = pan_run(h, w, fmt, N, A, d, 0, R * A)) return rc;
    if (rows) HIPCHK(h, hipMemcpyAsync(rows, w.d_ring, sizeof(float) * (size_t)R * (size_t)bins, hipMemcpyDeviceToHost, h->stream));
    if (stats) HIPCHK(h, hipMemcpyAsync(stats, w.d_rstat, sizeof(int32_t) * 2 * (size_t)R, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}
static int pan_n_check(ft8rx_handle* h, const char* who, uint64_t n_samples) {
    if (n_samples <= FT8RX_PAN_MAX_SAMPLES) return 0;
    set_err(h, "%s: n_samples %llu outside [0, %llu]", who, (unsigned long long)n_samples, (unsigned long long)FT8RX_PAN_MAX_SAMPLES);
    return -1;
}

int ft8rx_pan(ft8rx_handle* h, const void* d_samples, int kind, uint64_t n_samples, int n_fft, int n_avg, float* rows, int32_t* stats, uint64_t* n_rows_out) {
    if (!h) return -1;
    const int fmt = pan_check(h, "ft8rx_pan", kind, n_fft, n_avg);
    if (fmt < 0 || pan_n_check(h, "ft8rx_pan", n_samples)) return -1;
    if (!d_samples || ((uintptr_t)d_samples % sf_component_bytes(fmt)) != 0) { set_err(h, "ft8rx_pan: d_samples is NULL or not aligned to a component"); return -1; }
    ENTER(h);
    return pan_oneshot(h, "ft8rx_pan", (const char*)d_samples, fmt, n_samples, n_fft, n_avg, rows, stats, n_rows_out);
}

int ft8rx_pan_host(ft8rx_handle* h, const void* samples, int kind, uint64_t n_samples, int n_fft, int n_avg, float* rows, int32_t* stats, uint64_t* n_rows_out) {
    if (!h) return -1;
    const int fmt = pan_check(h, "ft8rx_pan_host", kind, n_fft, n_avg);
    if (fmt < 0 || pan_n_check(h, "ft8rx_pan_host", n_samples)) return -1;
    if (!samples) { set_err(h, "ft8rx_pan_host: samples is NULL"); return -1; }
    ENTER(h);
    const size_t bytes = (size_t)(n_samples / (uint64_t)n_fft / (uint64_t)n_avg) * (size_t)n_avg * (size_t)n_fft * sf_sample_bytes(fmt);      // whole rows only
    if (bytes) {
        if (grow_dev(h, "ft8rx_pan_host", &h->d_pan_in, &h->pan_in_cap, bytes)) return -2;
        HIPCHK(h, hipMemcpyAsync(h->d_pan_in, samples, bytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));         // the caller's memory is free again
    }
    return pan_oneshot(h, "ft8rx_pan_host", (const char*)h->d_pan_in, fmt, n_samples, n_fft, n_avg, rows, stats, n_rows_out);
}

static void pan_stream_release(ft8rx_handle* h) {
    ft8rx_handle::PanStream& s = h->pans;
    release_dev(h, s.d_work); release_dev(h, s.d_left); release_host(h, s.h_stage);
    release_dev(h, s.ws.d_win); release_dev(h, s.ws.d_pw); release_dev(h, s.ws.d_wstat); release_dev(h, s.ws.d_ring); release_dev(h, s.ws.d_rstat);
    const hipEvent_t ev = s.ev;
    s = ft8rx_handle::PanStream();
    s.ev = ev;
}

int ft8rx_pan_stream_open(ft8rx_handle* h, int kind, int n_fft, int n_avg, int n_rows, uint64_t n_origin, uint64_t max_push) {
    if (!h) return -1;
    const char* who = "ft8rx_pan_stream_open";
    if (h->pans.open) { set_err(h, "%s: a panorama stream is open on this handle already (ft8rx_pan_stream_close)", who); return -1; }
    const int fmt = pan_check(h, who, kind, n_fft, n_avg);
    if (fmt < 0) return -1;
    if (n_rows < 1 || n_rows > FT8RX_PAN_MAX_ROWS) { set_err(h, "%s: n_rows %d outside [1, %d]", who, n_rows, FT8RX_PAN_MAX_ROWS); return -1; }
    if (n_origin > ((uint64_t)1 << 53)) { set_err(h, "%s: n_origin %llu beyond 2^53", who, (unsigned long long)n_origin); return -1; }
    if (max_push < 1 || max_push > FT8RX_PAN_MAX_PUSH) {
        set_err(h, "%s: max_push %llu outside [1, %llu]", who, (unsigned long long)max_push, (unsigned long long)FT8RX_PAN_MAX_PUSH); return -1;
    }
    ENTER(h);
    if (pan_tables(h)) return -2;
    ft8rx_handle::PanStream& s = h->pans;
    const size_t sb = sf_sample_bytes(fmt);
    const int bins = sf_is_iq(fmt) ? n_fft : n_fft / 2;
    const size_t slots = (size_t)panring::slots(n_rows);
    const size_t tile = (size_t)panring::tile_windows((int64_t)pan_tile_cap(bins, (int64_t)(max_push / (uint64_t)n_fft) + 1), n_rows, n_avg);
    std::vector<float> win((size_t)n_fft);
    pan_window(n_fft, win.data());
    int rc = 0;
    hipError_t e = hipSuccess;
    if (!s.ev) e = hipEventCreateWithFlags(&s.ev, hipEventDisableTiming);
    if (e != hipSuccess) { set_err(h, "%s: %s", who, hipGetErrorString(e)); rc = -2; }
    if (!rc) rc = dalloc(h, &s.d_work, (size_t)panring::capacity(n_fft, (int64_t)max_push) * sb);
    if (!rc) rc = dalloc(h, &s.d_left, (size_t)n_fft * sb);
    if (!rc) rc = halloc(h, &s.h_stage, (size_t)max_push * sb);
    if (!rc) rc = dalloc(h, &s.ws.d_win, (size_t)n_fft);
    if (!rc) rc = dalloc(h, &s.ws.d_pw, tile * (size_t)bins);
    if (!rc) rc = dalloc(h, &s.ws.d_wstat, 2 * tile);
    if (!rc) rc = dalloc(h, &s.ws.d_ring, slots * (size_t)bins);
    if (!rc) rc = dalloc(h, &s.ws.d_rstat, 2 * slots);
    if (!rc && (e = hipMemcpy(s.ws.d_win, win.data(), sizeof(float) * win.size(), hipMemcpyHostToDevice)) != hipSuccess) { set_err(h, "%s: %s", who, hipGetErrorString(e)); rc = -2; }
    if (rc) { pan_stream_release(h); return -2; }
    s.ws.win_n = n_fft; s.ws.tile_w = tile; s.ws.slots = slots;
    s.fmt = fmt; s.N = n_fft; s.A = n_avg; s.n_rows = n_rows;
    s.n_origin = (int64_t)n_origin; s.pushed = 0; s.max_push = (int64_t)max_push; s.open = true;
    return 0;
}

int ft8rx_pan_stream_push(ft8rx_handle* h, const void* in, uint64_t n_new, int on_device, void** d_samples, uint64_t* rows_done) {
    if (!h) return -1;
    const char* who = "ft8rx_pan_stream_push";
    ft8rx_handle::PanStream& s = h->pans;
    if (!s.open) { set_err(h, "%s: no panorama stream is open (ft8rx_pan_stream_open)", who); return -1; }
    if (n_new > (uint64_t)s.max_push) { set_err(h, "%s: n_new %llu outside [0, %llu] (max_push)", who, (unsigned long long)n_new, (unsigned long long)s.max_push); return -1; }
    const size_t sb = sf_sample_bytes(s.fmt), align = sf_component_bytes(s.fmt);
    if (n_new && (!in || (on_device && ((uintptr_t)in % align) != 0))) { set_err(h, "%s: in is NULL or not aligned to a component", who); return -1; }
    if (s.n_origin + s.pushed + (int64_t)n_new > ((int64_t)1 << 54)) { set_err(h, "%s: n_new %llu takes the stream past index 2^54", who, (unsigned long long)n_new); return -1; }
    // (no ENTER: a push touches the stream's own buffers only, on the main stream; batches in flight read none of them)
    HIPCHK(h, hipSetDevice(h->device));
    const panring::Plan p = panring::plan(s.n_origin, s.n_origin + s.pushed, (int64_t)n_new, s.N, s.A);
    // [leftover | chunk]: behind whatever read the last chunk from this buffer (the front end's device push is on the same stream)
    if (p.left_n > 0) HIPCHK(h, hipMemcpyAsync(s.d_work, s.d_left, (size_t)p.left_n * sb, hipMemcpyDeviceToDevice, h->stream));
    char* dst = s.d_work + (size_t)p.chunk_at * sb;
    if (n_new) {
        if (on_device) {
            HIPCHK(h, hipMemcpyAsync(dst, in, (size_t)n_new * sb, hipMemcpyDeviceToDevice, h->stream));
        } else {                                         // through the page-locked buffer, once the previous push's copy has left it
            HIPCHK(h, hipEventSynchronize(s.ev));
            memcpy(s.h_stage, in, (size_t)n_new * sb);
            HIPCHK(h, hipMemcpyAsync(dst, s.h_stage, (size_t)n_new * sb, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipEventRecord(s.ev, h->stream));
        }
    }
    if (p.w1 > p.w0)
        if (const int rc = pan_run(h, s.ws, s.fmt, s.N, s.A, s.d_work + (size_t)p.first_at * sb, p.w0, p.w1 - p.w0)) return rc;
    if (p.keep_n > 0) HIPCHK(h, hipMemcpyAsync(s.d_left, s.d_work + (size_t)p.keep_at * sb, (size_t)p.keep_n * sb, hipMemcpyDeviceToDevice, h->stream));
    s.pushed += (int64_t)n_new;
    if (d_samples) *d_samples = dst;
    if (rows_done) *rows_done = (uint64_t)p.r1;
    return 0;
}

int ft8rx_pan_stream_read(ft8rx_handle* h, uint64_t r_first, int n, float* rows, int32_t* stats) {
    if (!h) return -1;
    const char* who = "ft8rx_pan_stream_read";
    const ft8rx_handle::PanStream& s = h->pans;
    if (!s.open) { set_err(h, "%s: no panorama stream is open (ft8rx_pan_stream_open)", who); return -1; }
    const panring::Held held = panring::held(s.n_origin, s.n_origin + s.pushed, s.N, s.A, s.n_rows);
    if (n < 0 || (int64_t)r_first < held.r_lo || r_first > (uint64_t)held.r_hi || (int64_t)r_first + n > held.r_hi) {
        set_err(h, "%s: r_first %llu, n %d: the ring holds the rows [%lld, %lld)", who, (unsigned long long)r_first, n, (long long)held.r_lo, (long long)held.r_hi);
        return -1;
    }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t bins = sf_is_iq(s.fmt) ? (size_t)s.N : (size_t)s.N / 2;
    for (int i = 0; i < n;) {                            // in runs that do not wrap
        const size_t slot = (size_t)((r_first + (uint64_t)i) % s.ws.slots);
        const int run = (size_t)(n - i) < s.ws.slots - slot ? n - i : (int)(s.ws.slots - slot);
        if (rows) HIPCHK(h, hipMemcpyAsync(rows + (size_t)i * bins, s.ws.d_ring + slot * bins, sizeof(float) * (size_t)run * bins, hipMemcpyDeviceToHost, h->stream));
        if (stats) HIPCHK(h, hipMemcpyAsync(stats + 2 * (size_t)i, s.ws.d_rstat + 2 * slot, sizeof(int32_t) * 2 * (size_t)run, hipMemcpyDeviceToHost, h->stream));
        i += run;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int ft8rx_pan_stream_info(ft8rx_handle* h, uint64_t* n_pushed, uint64_t* rows_done, uint64_t* r_lo, int* bins) {
    if (!h) return -1;
    const ft8rx_handle::PanStream& s = h->pans;
    if (!s.open) { set_err(h, "ft8rx_pan_stream_info: no panorama stream is open (ft8rx_pan_stream_open)"); return -1; }
    const panring::Held held = panring::held(s.n_origin, s.n_origin + s.pushed, s.N, s.A, s.n_rows);
    if (n_pushed) *n_pushed = (uint64_t)s.pushed;
    if (rows_done) *rows_done = (uint64_t)held.r_hi;
    if (r_lo) *r_lo = (uint64_t)held.r_lo;
    if (bins) *bins = sf_is_iq(s.fmt) ? s.N : s.N / 2;
    return 0;
}

int ft8rx_pan_stream_close(ft8rx_handle* h) {
    if (!h) return -1;
    if (!h->pans.open) { set_err(h, "ft8rx_pan_stream_close: no panorama stream is open"); return -1; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));          // pushes, and what read the chunk from the work buffer
    pan_stream_release(h);
    return 0;
}

int ft8rx_set_search_mask(ft8rx_handle* h, const uint8_t* mask, int n_frames) {
    if (!h) return -1;
    ENTER(h);                                   // batches in flight were enqueued under the previous setting
    if (!mask) { h->use_mask = false; return 0; }
    if (n_frames < 1 || n_frames > h->max_frames) { set_err(h, "ft8rx_set_search_mask: n_frames %d outside [1, %d]", n_frames, h->max_frames); return -1; }
    if (!ws_ready(h, WS_MASK)) {
        FirstUse F(h, WS_MASK);
        F.dev(&h->d_colmask, (size_t)h->max_frames * NF0MAX);
        if (F.done()) return -2;
    }
    const int nf0 = h->cfg.f0_hi - h->cfg.f0_lo;
    HIPCHK(h, hipMemsetAsync(h->d_colmask, 0, (size_t)h->max_frames * NF0MAX, h->stream));
    HIPCHK(h, hipMemcpy2DAsync(h->d_colmask, NF0MAX, mask, (size_t)nf0, (size_t)nf0, n_frames, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->use_mask = true;
    return 0;
}

int ft8rx_sync(ft8rx_handle* h) {
    if (!h) return -1;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipStreamSynchronize(h->copy_s));
    if (h->profiling && !h->pnames.empty()) {
        h->n_stage = (int)h->pnames.size();
        for (int i = 0; i < h->n_stage; i++) hipEventElapsedTime(&h->stage_ms[i], h->pev[i], h->pev[i + 1]);
    }
    return 0;
}

// The batch a fetch hands out: the oldest unfetched one, else the latest one again, once its results have reached the host buffers
// (with_events: and its event log lies in h_ev's rows).  to_device (ft8rx_results_to_device): always the latest one, as soon as its
// kernels are done on every chunk stream (the results sit in the slot's device buffers).  -> 0 and *slot, or the error code
static int fetch_begin(ft8rx_handle* h, const char* who, int B, bool with_events, bool to_device, int* slot) {
    if (!h || B < 1 || B > h->max_frames) return -1;
    if (h->last_slot < 0) { set_err(h, "%s: nothing has been enqueued", who); return -1; }
    HIPCHK(h, hipSetDevice(h->device));
    *slot = (h->inflight && !to_device) ? h->slot_fetch : h->last_slot;
    ResultSlot& sl = h->slots[*slot];
    if (B > sl.B) { set_err(h, "%s: %d frames requested, the batch had %d", who, B, sl.B); return -1; }
    HIPCHK(h, hipEventSynchronize(to_device ? sl.ev_comp : sl.ev_done));
    if (with_events && !to_device) fetch_events(sl);
    return 0;
}
static void fetch_end(ft8rx_handle* h, int slot) {
    h->fetched_slot = slot;
    if (h->inflight) { h->slot_fetch ^= 1; h->inflight--; }
}

int ft8rx_fetch_results(ft8rx_handle* h, int B, ft8rx_record* records, int32_t* counts, ft8rx_event* events, int32_t* event_counts) {
    int slot;
    if (const int rc = fetch_begin(h, "ft8rx_fetch_results", B, events != nullptr, false, &slot)) return rc;
    const ResultSlot& sl = h->slots[slot];
    const size_t mc = (size_t)h->cfg.max_cands;
    if (counts) memcpy(counts, sl.h_cnt, sizeof(int32_t) * B);
    if (records) memcpy(records, sl.h_rec, sizeof(ft8rx_record) * mc * B);
    if (event_counts) memcpy(event_counts, sl.h_evc, sizeof(int32_t) * B);
    if (events) for (int f = 0; f < B; f++) {              // the used entries of each frame; the rest of the caller's row is left alone
        int c = sl.h_evc[f]; if (c > FT8RX_EVENT_CAP) c = FT8RX_EVENT_CAP;
        if (c > 0) memcpy(events + (size_t)f * FT8RX_EVENT_CAP, sl.h_ev + (size_t)f * FT8RX_EVENT_CAP, sizeof(ft8rx_event) * (size_t)c);
    }
    fetch_end(h, slot);
    return 0;
}

int ft8rx_fetch_results_view(ft8rx_handle* h, int B, const ft8rx_record** records, const int32_t** counts,
                             const ft8rx_event** events, const int32_t** event_counts) {
    int slot;
    if (const int rc = fetch_begin(h, "ft8rx_fetch_results_view", B, events != nullptr, false, &slot)) return rc;
    const ResultSlot& sl = h->slots[slot];
    if (records) *records = sl.h_rec;
    if (counts) *counts = sl.h_cnt;
    if (events) *events = sl.h_ev;
    if (event_counts) *event_counts = sl.h_evc;
    fetch_end(h, slot);
    return 0;
}

int ft8rx_set_packed_output(ft8rx_handle* h, void* d_buf0, void* d_buf1, uint64_t cap_bytes) {
    if (!h) return -1;
    ENTER(h);                                   // batches in flight keep the buffers they were enqueued with
    HIPCHK(h, hipStreamSynchronize(h->copy_s));
    ResultSlot* const sl = h->slots;
    sl[0].pk_fence = sl[1].pk_fence = nullptr;
    if (!d_buf0 && !d_buf1) { sl[0].pk_buf = sl[1].pk_buf = nullptr; h->pk_cap = 0; return 0; }
    if (refuse_conflict(h, "ft8rx_set_packed_output", optins::PACKED)) return -1;
    if (!d_buf0 || !d_buf1 || d_buf0 == d_buf1 || cap_bytes < sizeof(ft8rx_packed_header)) {
        set_err(h, "ft8rx_set_packed_output: two distinct buffers of at least %zu bytes each are needed", sizeof(ft8rx_packed_header)); return -1; }
    void* in[2] = {d_buf0, d_buf1};
    unsigned char* dev[2];
    for (int k = 0; k < 2; k++) {               // page-locked host memory is addressed through its device pointer
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, in[k]) != hipSuccess) { (void)hipGetLastError(); set_err(h, "ft8rx_set_packed_output: buffer %d is neither device nor page-locked host memory", k); return -1; }
        if (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeHost && at.type != hipMemoryTypeManaged) {      // e.g. plain malloc memory: the kernels could not write it
            set_err(h, "ft8rx_set_packed_output: buffer %d is ordinary host memory; use device memory or ft8rx_alloc_host", k); return -1; }
        dev[k] = (unsigned char*)(at.type == hipMemoryTypeHost ? at.devicePointer : in[k]);
        if (!dev[k] || ((uintptr_t)dev[k] & 15)) { set_err(h, "ft8rx_set_packed_output: buffer %d is not device-accessible / 16-byte aligned", k); return -1; }
    }
    if (!ws_ready(h, WS_PACKED)) {
        FirstUse F(h, WS_PACKED);
        F.dev(&h->d_pkneed, (size_t)h->max_frames * ((1 << cand_shift(h->cfg)) / 64));      // k_pack_count's mask words
        F.dev(&h->d_pknrec, (size_t)h->max_frames);
        for (int k = 0; k < 2; k++) F.host(&sl[k].h_pkhdr, 1, &sl[k].d_pkhdr);
        if (F.done()) return -2;
        for (int k = 0; k < 2; k++) memset(sl[k].h_pkhdr, 0, sizeof(ft8rx_packed_header));
    }
    sl[0].pk_buf = dev[0]; sl[1].pk_buf = dev[1]; h->pk_cap = cap_bytes;
    return 0;
}

int ft8rx_packed_output_fence(ft8rx_handle* h, int which, void* hip_event) {
    if (!h || which < 0 || which > 1) return -1;
    h->slots[which].pk_fence = (hipEvent_t)hip_event;
    return 0;
}

int ft8rx_packed_results(ft8rx_handle* h, int32_t* which, ft8rx_packed_header* header) {
    if (!h) return -1;
    if (h->fetched_slot < 0 || !h->slots[h->fetched_slot].packed) { set_err(h, "ft8rx_packed_results: the batch fetched last was enqueued without a packed output (ft8rx_set_packed_output)"); return -1; }
    if (which) *which = h->fetched_slot;
    if (header) *header = *h->slots[h->fetched_slot].h_pkhdr;
    return 0;
}

int ft8rx_results_to_device(ft8rx_handle* h, int B, ft8rx_record* d_records, int32_t* d_counts, ft8rx_event* d_events, int32_t* d_event_counts) {
    int slot;
    if (const int rc = fetch_begin(h, "ft8rx_results_to_device", B, false, true, &slot)) return rc;
    const ResultSlot& sl = h->slots[slot];
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int mc = h->cfg.max_cands;
    if (d_counts) HIPCHK(h, hipMemcpyAsync(d_counts, sl.ncand, sizeof(int32_t) * B, hipMemcpyDeviceToDevice, h->stream));
    if (d_records) HIPCHK(h, hipMemcpy2DAsync(d_records, sizeof(ft8rx_record) * mc, sl.rec, sizeof(ft8rx_record) << cand_shift(h->cfg),
                                              sizeof(ft8rx_record) * mc, B, hipMemcpyDeviceToDevice, h->stream));
    if (d_event_counts) HIPCHK(h, hipMemcpyAsync(d_event_counts, sl.evcount, sizeof(int32_t) * B, hipMemcpyDeviceToDevice, h->stream));
    if (d_events) HIPCHK(h, hipMemcpyAsync(d_events, sl.ev, sizeof(ft8rx_event) * (size_t)B * FT8RX_EVENT_CAP, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// the synchronous host entries: nothing older is kept, and the audio is staged in the handle's own buffer
static int launch_batch_sync(ft8rx_handle* h, const Frames& audio, int B) {
    h->inflight = 0; h->slot_fetch = h->slot_enq;
    if (need_staging(h, audio.sb, false)) return -2;
    return launch_batch(h, batchplan::HOST_SYNC, audio, B);
}

int ft8rx_decode_batch(ft8rx_handle* h, const int16_t* audio, int B, ft8rx_record* records, int32_t* counts,
                       ft8rx_event* events, int32_t* event_counts) {
    if (!h || !audio) return -1;
    if (B < 1 || B > h->max_frames) { set_err(h, "ft8rx_decode_batch: n_frames %d outside [1, %d]", B, h->max_frames); return -1; }
    if (const int rc = launch_batch_sync(h, Frames{audio, 2}, B)) return rc;
    return ft8rx_fetch_results(h, B, records, counts, events, event_counts);
}
int ft8rx_decode_batch_f32(ft8rx_handle* h, const float* audio, int B, ft8rx_record* records, int32_t* counts,
                           ft8rx_event* events, int32_t* event_counts) {
    if (!h || !audio) return -1;
    if (B < 1 || B > h->max_frames) { set_err(h, "ft8rx_decode_batch_f32: n_frames %d outside [1, %d]", B, h->max_frames); return -1; }
    if (const int rc = launch_batch_sync(h, Frames{audio, 4}, B)) return rc;
    return ft8rx_fetch_results(h, B, records, counts, events, event_counts);
}

// One call from host audio to rendered messages: ft8rx_decode_batch + ft8rx_package_batch without the intermediate copies (the
// packager reads the handle's page-locked result buffers in place).
static int decode_messages(ft8rx_handle* h, const char* who, const Frames& audio, int B, ft8rx_message* out, int max_msgs, int32_t* out_counts,
                           int n_threads, ft8rx_hashes* table, int32_t* flags) {
    if (!h || !audio.p || !out || !out_counts) return -1;
    if (B < 1 || B > h->max_frames || max_msgs < 1) { set_err(h, "%s: bad n_frames / max_msgs", who); return -1; }
    if (refuse_conflict(h, who, optins::DECODE_MESSAGES,
                        " (ft8rx_message rows cannot carry it); use ft8rx_decode_batch with ft8rx_package_batch_ext / ft8rx_fetch_recall")) return -1;
    int rc = launch_batch_sync(h, audio, B);
    if (rc) return rc;
    const ft8rx_record* rec; const int32_t* cnt; const ft8rx_event* ev; const int32_t* evc;
    rc = ft8rx_fetch_results_view(h, B, &rec, &cnt, &ev, &evc);
    if (rc) return rc;
    return hostmsg::package_batch(rec, cnt, ev, evc, B, h->cfg.max_cands, out, max_msgs, out_counts, n_threads, table ? &table->H : nullptr, flags);
}
int ft8rx_decode_messages(ft8rx_handle* h, const int16_t* audio, int B, ft8rx_message* out, int max_msgs, int32_t* out_counts,
                          int n_threads, ft8rx_hashes* table, int32_t* flags) {
    return decode_messages(h, "ft8rx_decode_messages", Frames{audio, 2}, B, out, max_msgs, out_counts, n_threads, table, flags);
}
int ft8rx_decode_messages_f32(ft8rx_handle* h, const float* audio, int B, ft8rx_message* out, int max_msgs, int32_t* out_counts,
                              int n_threads, ft8rx_hashes* table, int32_t* flags) {
    return decode_messages(h, "ft8rx_decode_messages_f32", Frames{audio, 4}, B, out, max_msgs, out_counts, n_threads, table, flags);
}

// ---------------------------------------------------------------------------- stage entry points
#define NEED(p) do { if (!(p)) { set_err(h, "scratch allocation/copy failed (%s:%d)", __FILE__, __LINE__); return -2; } } while (0)

// host frames -> the staging buffer of their sample form (*d: the frames there)
static int stage_frames(ft8rx_handle* h, const Frames& audio, int B, Frames* d) {
    if (need_staging(h, audio.sb, false)) return -2;
    *d = Frames{staging_of(h, audio.sb, false), audio.sb};
    HIPCHK(h, hipMemcpy(const_cast<void*>(d->p), audio.p, audio.bytes((size_t)B), hipMemcpyHostToDevice));
    return 0;
}
static int spectrogram_entry(ft8rx_handle* h, const Frames& audio, int B, float* grid) {
    if (!h || !audio.p || !grid || B < 1 || B > h->max_frames) return -1;
    ENTER(h);
    Frames d;
    if (const int rc = stage_frames(h, audio, B, &d)) return rc;
    launch_spectrogram(B, h->stream, d, h->d_grid, h->T);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(grid, h->d_grid, sizeof(float) * (size_t)B * FT8RX_GRID_ROWS * FT8RX_GRID_COLS, hipMemcpyDeviceToHost));
    return 0;
}
int ft8rx_spectrogram(ft8rx_handle* h, const int16_t* audio, int B, float* grid) { return spectrogram_entry(h, Frames{audio, 2}, B, grid); }
int ft8rx_spectrogram_f32(ft8rx_handle* h, const float* audio, int B, float* grid) { return spectrogram_entry(h, Frames{audio, 4}, B, grid); }

int ft8rx_hop_spectrum(ft8rx_handle* h, const int16_t* window3840, float* row) {
    if (!h || !window3840 || !row) return -1;
    ENTER(h);
    if (need_staging(h)) return -2;
    float* d_row = h->d_best_score;                      // any scratch of FT8RX_GRID_COLS floats (NF0MAX >= that): not in use between batches
    HIPCHK(h, hipMemcpyAsync(h->d_audio, window3840, sizeof(int16_t) * 3840, hipMemcpyHostToDevice, h->stream));
    ft8rx_ilp_hop_spectrum(h->stream, h->d_audio, d_row, h->T);
    HIPCHK(h, hipMemcpyAsync(row, d_row, sizeof(float) * FT8RX_GRID_COLS, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int ft8rx_sync_search(ft8rx_handle* h, const float* grid, int B, int32_t* f0_idx, int32_t* h0_idx, float* score, int32_t* counts) {
    if (!h || !grid || B < 1 || B > h->max_frames) return -1;
    ENTER(h);
    const ft8rx_config& c = h->cfg;
    HIPCHK(h, hipMemcpy(h->d_grid, grid, sizeof(float) * (size_t)B * FT8RX_GRID_ROWS * FT8RX_GRID_COLS, hipMemcpyHostToDevice));
    launch_sync(h->d_grid, h->d_best_score, h->d_best_h0, c, B, h->stream, false);
    k_topk<<<B, 1024, 0, h->stream>>>(h->d_best_score, h->d_best_h0, h->d_rec, h->d_ncand, c, nullptr, nullptr, nullptr);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t S = (size_t)1 << cand_shift(c);
    std::vector<ft8rx_record> rec((size_t)B * S);
    HIPCHK(h, hipMemcpy(rec.data(), h->d_rec, sizeof(ft8rx_record) * rec.size(), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(counts, h->d_ncand, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    for (int f = 0; f < B; f++) for (int i = 0; i < c.max_cands; i++) {
        const ft8rx_record& r = rec[(size_t)f * S + i];
        size_t o = (size_t)f * c.max_cands + i;
        f0_idx[o] = r.f0_idx; h0_idx[o] = r.h0_idx; score[o] = r.score;
    }
    return 0;
}

static int sync_scores(ft8rx_handle* h, const float* grid, int B, int f0_lo, int f0_hi, float* score, int32_t* h0_idx, bool weak) {
    const char* who = weak ? "ft8rx_sync_scores_weak" : "ft8rx_sync_scores";
    if (!h || !grid || !score || !h0_idx || B < 1 || B > h->max_frames) return -1;
    if (f0_lo < 4 || f0_hi <= f0_lo || f0_hi > FT8RX_GRID_COLS - 15 || f0_hi - f0_lo > NF0MAX) {
        set_err(h, "%s: f0 range [%d, %d) outside [4, %d]", who, f0_lo, f0_hi, FT8RX_GRID_COLS - 15); return -1; }
    ENTER(h);
    ft8rx_config c = h->cfg;
    c.f0_lo = f0_lo; c.f0_hi = f0_hi;
    HIPCHK(h, hipMemcpy(h->d_grid, grid, sizeof(float) * (size_t)B * FT8RX_GRID_ROWS * FT8RX_GRID_COLS, hipMemcpyHostToDevice));
    const int nf0 = f0_hi - f0_lo;
    launch_sync(h->d_grid, h->d_best_score, h->d_best_h0, c, B, h->stream, weak);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpy2DAsync(score, sizeof(float) * nf0, h->d_best_score, sizeof(float) * NF0MAX, sizeof(float) * nf0, B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpy2DAsync(h0_idx, sizeof(int32_t) * nf0, h->d_best_h0, sizeof(int32_t) * NF0MAX, sizeof(int32_t) * nf0, B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int ft8rx_sync_scores(ft8rx_handle* h, const float* grid, int B, int f0_lo, int f0_hi, float* score, int32_t* h0_idx) {
    return sync_scores(h, grid, B, f0_lo, f0_hi, score, h0_idx, false);
}
int ft8rx_sync_scores_weak(ft8rx_handle* h, const float* grid, int B, int f0_lo, int f0_hi, float* score, int32_t* h0_idx) {
    return sync_scores(h, grid, B, f0_lo, f0_hi, score, h0_idx, true);
}

// the (frame, f0, h0) triples of a stage entry, interleaved as the kernels' test entries read them
static std::vector<int32_t> pack_triples(int n, const int32_t* frame, const int32_t* f0_idx, const int32_t* h0_idx) {
    std::vector<int32_t> trip(3 * (size_t)n);
    for (int i = 0; i < n; i++) { trip[3 * i] = frame[i]; trip[3 * i + 1] = f0_idx[i]; trip[3 * i + 2] = h0_idx[i]; }
    return trip;
}

int ft8rx_llr_grid(ft8rx_handle* h, const float* grid, int B, int n, const int32_t* frame, const int32_t* f0_idx,
                   const int32_t* h0_idx, float* llr, float* sd, int32_t* snr) {
    if (!h || !grid || B < 1 || B > h->max_frames || n < 1) return -1;
    ENTER(h);
    HIPCHK(h, hipMemcpy(h->d_grid, grid, sizeof(float) * (size_t)B * FT8RX_GRID_ROWS * FT8RX_GRID_COLS, hipMemcpyHostToDevice));
    const std::vector<int32_t> trip = pack_triples(n, frame, f0_idx, h0_idx);
    Scratch S{h};
    int32_t* d_trip = S.put(trip.data(), trip.size()); NEED(d_trip);
    float* d_llr = S.get<float>((size_t)n * 174); NEED(d_llr);
    float* d_sd = S.get<float>(n); NEED(d_sd);
    int32_t* d_snr = S.get<int32_t>(n); NEED(d_snr);
    k_grid_llr<<<n, 64, 0, h->stream>>>(h->d_grid, nullptr, nullptr, d_llr, h->cfg, d_trip, d_sd, d_snr, nullptr, nullptr, nullptr, n);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(llr, d_llr, sizeof(float) * (size_t)n * 174, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(sd, d_sd, sizeof(float) * n, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(snr, d_snr, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return 0;
}

static int cycle_spectrum_entry(ft8rx_handle* h, const Frames& audio, int B, float* spec) {
    if (!h || !audio.p || !spec || B < 1 || B > h->max_frames) return -1;
    ENTER(h);
    Frames d;
    if (const int rc = stage_frames(h, audio, B, &d)) return rc;
    launch_cyc_a(B, h->stream, d, h->d_A, h->T);
    k_cyc_bc<<<dim3(CYC_BC_GRID, B), 256, 0, h->stream>>>(h->d_A, h->d_spec, h->T);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(spec, h->d_spec, sizeof(cpx) * (size_t)B * FT8RX_SPEC_BINS, hipMemcpyDeviceToHost));
    return 0;
}
int ft8rx_cycle_spectrum(ft8rx_handle* h, const int16_t* audio, int B, float* spec) { return cycle_spectrum_entry(h, Frames{audio, 2}, B, spec); }
int ft8rx_cycle_spectrum_f32(ft8rx_handle* h, const float* audio, int B, float* spec) { return cycle_spectrum_entry(h, Frames{audio, 4}, B, spec); }

static int fine_probe(ft8rx_handle* h, const float* spec, int B, int n, const int32_t* frame, const int32_t* f0_idx, const int32_t* h0_idx,
                      int32_t* ret, int32_t* ttweak, int32_t* ftweak, int32_t* nsync, float* llr, float* sd, int32_t* snr, float* sgrid, bool weak) {
    if (!h || !spec || B < 1 || B > h->max_frames || n < 1) return -1;
    // weak mode only (ft8rx_fine keeps its unchecked contract): every triple must name a frame of the spectrum and a candidate the
    // search could give
    if (weak) for (int i = 0; i < n; i++)
        if (frame[i] < 0 || frame[i] >= B || f0_idx[i] < 4 || f0_idx[i] >= FT8RX_MAX_F0 || h0_idx[i] < FT8RX_MIN_H0 || h0_idx[i] >= FT8RX_MAX_H0) {
            set_err(h, "ft8rx_fine_weak: triple %d (frame %d, f0 %d, h0 %d) outside [0, %d) x [4, %d) x [%d, %d)", i,
                    frame[i], f0_idx[i], h0_idx[i], B, FT8RX_MAX_F0, FT8RX_MIN_H0, FT8RX_MAX_H0); return -1; }
    ENTER(h);
    HIPCHK(h, hipMemcpy(h->d_spec, spec, sizeof(cpx) * (size_t)B * FT8RX_SPEC_BINS, hipMemcpyHostToDevice));
    const std::vector<int32_t> trip = pack_triples(n, frame, f0_idx, h0_idx);
    Scratch S{h};
    int32_t* d_trip = S.put(trip.data(), trip.size()); NEED(d_trip);
    float* d_llr = S.get<float>((size_t)n * 174); NEED(d_llr);
    HIPCHK(h, hipMemset(d_llr, 0, sizeof(float) * (size_t)n * 174));
    float* d_sd = S.get<float>(n); NEED(d_sd);
    int32_t* d_out = S.get<int32_t>((size_t)n * 5); NEED(d_out);
    float* d_sg = sgrid ? S.get<float>((size_t)n * 632) : nullptr; if (sgrid) NEED(d_sg);
    launch_fine(h, weak ? weak_config(h) : h->cfg, weak, n, h->stream, h->d_spec, nullptr, nullptr, d_llr, d_trip, d_out, d_sd, d_sg,
                WorkList{nullptr, nullptr}, true);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<int32_t> o((size_t)n * 5);
    HIPCHK(h, hipMemcpy(o.data(), d_out, sizeof(int32_t) * o.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) { ret[i] = o[5 * i]; ttweak[i] = o[5 * i + 1]; ftweak[i] = o[5 * i + 2]; nsync[i] = o[5 * i + 3]; snr[i] = o[5 * i + 4]; }
    HIPCHK(h, hipMemcpy(llr, d_llr, sizeof(float) * (size_t)n * 174, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(sd, d_sd, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (sgrid) HIPCHK(h, hipMemcpy(sgrid, d_sg, sizeof(float) * (size_t)n * 632, hipMemcpyDeviceToHost));
    return 0;
}

int ft8rx_fine(ft8rx_handle* h, const float* spec, int B, int n, const int32_t* frame, const int32_t* f0_idx, const int32_t* h0_idx,
               int32_t* ret, int32_t* ttweak, int32_t* ftweak, int32_t* nsync, float* llr, float* sd, int32_t* snr, float* sgrid) {
    return fine_probe(h, spec, B, n, frame, f0_idx, h0_idx, ret, ttweak, ftweak, nsync, llr, sd, snr, sgrid, false);
}
int ft8rx_fine_weak(ft8rx_handle* h, const float* spec, int B, int n, const int32_t* frame, const int32_t* f0_idx, const int32_t* h0_idx,
                    int32_t* ret, int32_t* ttweak, int32_t* ftweak, int32_t* nsync, float* llr, float* sd, int32_t* snr, float* sgrid) {
    return fine_probe(h, spec, B, n, frame, f0_idx, h0_idx, ret, ttweak, ftweak, nsync, llr, sd, snr, sgrid, true);
}

int ft8rx_ldpc(ft8rx_handle* h, const float* llr, int n, int max_ncheck0, int max_iters, int32_t* ok, uint64_t* msg_lo,
               uint64_t* msg_hi, int32_t* n_its, int32_t* has_out, float* llr_out) {
    if (!h || !llr || n < 1) return -1;
    ENTER(h);
    Scratch S{h};
    float* d_in = S.put(llr, (size_t)n * 174); NEED(d_in);
    float* d_out = S.get<float>((size_t)n * 174); NEED(d_out);
    HIPCHK(h, hipMemset(d_out, 0, sizeof(float) * (size_t)n * 174));
    Att* d_att = S.get<Att>(n); NEED(d_att);
    k_bp<<<n, 64, 0, h->stream>>>(2, d_in, nullptr, nullptr, nullptr, d_att, d_out, nullptr, nullptr, h->cfg, max_ncheck0, max_iters, WorkList{nullptr, nullptr}, 0, 1);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<Att> a(n);
    HIPCHK(h, hipMemcpy(a.data(), d_att, sizeof(Att) * n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) { ok[i] = a[i].ok; msg_lo[i] = a[i].lo; msg_hi[i] = a[i].hi; n_its[i] = a[i].ok ? a[i].n_its : -1; has_out[i] = a[i].has_out; }
    if (llr_out) HIPCHK(h, hipMemcpy(llr_out, d_out, sizeof(float) * (size_t)n * 174, hipMemcpyDeviceToHost));
    return 0;
}

// ipass 7 alone, on n <= max_cands fine-LLR vectors of one frame (candidates 0 .. n - 1, each as the ladder leaves an undecoded one):
// the batch's launch sequence (launch_ap_calls) with the handle's setting -> their records and the frame's event log
int ft8rx_ap_calls_probe(ft8rx_handle* h, const float* llr, int n, ft8rx_record* records, ft8rx_event* events, int32_t* event_count) {
    if (!h || !llr || !records || n < 1 || n > h->cfg.max_cands) { if (h) set_err(h, "ft8rx_ap_calls_probe: 1 <= n <= max_cands"); return -1; }
    if (!h->ap.np) { set_err(h, "ft8rx_ap_calls_probe: no call set (ft8rx_set_ap_calls)"); return -1; }
    ENTER(h);
    Scratch S{h};
    const size_t st = (size_t)1 << cand_shift(h->cfg);
    std::vector<ft8rx_record> r0(st);
    memset(r0.data(), 0, sizeof(ft8rx_record) * st);
    for (int i = 0; i < n; i++) r0[i].status = FT8RX_ST_EXHAUSTED;
    std::vector<float> l0(st * 174, 0.0f);
    memcpy(l0.data(), llr, sizeof(float) * (size_t)n * 174);
    const int32_t nc = n, zero = 0;
    float* d_llr = S.put(l0.data(), l0.size()); NEED(d_llr);
    ft8rx_record* d_rec = S.put(r0.data(), st); NEED(d_rec);
    int32_t* d_nc = S.put(&nc, 1); NEED(d_nc);
    int32_t* d_evc = S.put(&zero, 1); NEED(d_evc);
    Att* d_att = S.get<Att>(st * 10); NEED(d_att);
    ft8rx_event* d_ev = S.get<ft8rx_event>(FT8RX_EVENT_CAP); NEED(d_ev);
    int32_t* d_cl = S.get<int32_t>(st); NEED(d_cl);
    int32_t* d_ol = S.get<int32_t>(st * 3); NEED(d_ol);
    int32_t* d_ac = S.get<int32_t>(2); NEED(d_ac);
    ApCalls* d_apc = S.get<ApCalls>(1); NEED(d_apc);
    k_ap_stage<<<1, 64, 0, h->stream>>>(d_apc, h->ap);
    launch_ap_calls(h, 1, d_llr, d_rec, d_nc, d_att, d_ev, d_evc, d_cl, d_ol, d_ac, d_apc, h->stream);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(records, d_rec, sizeof(ft8rx_record) * (size_t)n, hipMemcpyDeviceToHost));
    int32_t ne = 0;
    HIPCHK(h, hipMemcpy(&ne, d_evc, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (event_count) *event_count = ne;
    if (events) HIPCHK(h, hipMemcpy(events, d_ev, sizeof(ft8rx_event) * (size_t)(ne < FT8RX_EVENT_CAP ? ne : FT8RX_EVENT_CAP), hipMemcpyDeviceToHost));
    return 0;
}

// k_recall_score alone on caller-supplied fine grids: entry i is frame i's only entry, no ladder records (no skip rule), tweaks 0
int ft8rx_recall_probe(ft8rx_handle* h, const float* sgrid, const ft8rx_recall_entry* entries, int n, ft8rx_record* records) {
    if (!h || !sgrid || !entries || !records || n < 1) { if (h) set_err(h, "ft8rx_recall_probe: bad arguments"); return -1; }
    ENTER(h);
    Scratch S{h};
    std::vector<ft8rx_recall_entry> st((size_t)n * FT8RX_RECALL_MAX);
    std::vector<int32_t> trip(3 * (size_t)n), off(n + 1), tout(5 * (size_t)n, 0);
    for (int i = 0; i < n; i++) {
        ft8rx_recall_entry E = entries[i];
        E.pad = (uint16_t)recall_kind(E.msg_lo, E.msg_hi);
        st[(size_t)i * FT8RX_RECALL_MAX] = E;
        trip[3 * i] = i; trip[3 * i + 1] = E.f0_idx; trip[3 * i + 2] = E.h0_idx; off[i] = i;
    }
    off[n] = n;
    float* d_sg = S.put(sgrid, (size_t)n * 632); NEED(d_sg);
    ft8rx_recall_entry* d_ent = S.put(st.data(), st.size()); NEED(d_ent);
    int32_t* d_trip = S.put(trip.data(), trip.size()); NEED(d_trip);
    int32_t* d_off = S.put(off.data(), off.size()); NEED(d_off);
    int32_t* d_tout = S.put(tout.data(), tout.size()); NEED(d_tout);
    ft8rx_record* d_rec = S.get<ft8rx_record>((size_t)n * FT8RX_RECALL_MAX); NEED(d_rec);
    HIPCHK(h, hipMemset(d_rec, 0, sizeof(ft8rx_record) * (size_t)n * FT8RX_RECALL_MAX));
    k_recall_score<<<n, 64, 0, h->stream>>>(d_sg, d_tout, d_trip, d_off, 0, d_ent, nullptr, nullptr, 0, h->rc_max_hd, h->rc_min_gap, d_rec);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy2D(records, sizeof(ft8rx_record), d_rec, sizeof(ft8rx_record) * FT8RX_RECALL_MAX, sizeof(ft8rx_record), n, hipMemcpyDeviceToHost));
    return 0;
}

// the measurement step alone (launch_reports, as the batch chain runs it) on caller-supplied spectra: the candidates of frame f take the
// slots 0 .. of that frame's records, each DECODED with the given position, tweaks and word
int ft8rx_report_probe(ft8rx_handle* h, const float* spec, int B, int n, const int32_t* frame, const int32_t* f0_idx, const int32_t* h0_idx,
                       const int32_t* ttweak, const int32_t* ftweak, const uint64_t* msg_lo, const uint64_t* msg_hi, ft8rx_report* reports) {
    if (!h || !spec || !frame || !f0_idx || !h0_idx || !ttweak || !ftweak || !msg_lo || !msg_hi || !reports || B < 1 || B > h->max_frames || n < 1) {
        if (h) set_err(h, "ft8rx_report_probe: bad arguments (1 <= n_frames <= max_frames, n >= 1)"); return -1; }
    const int sh = cand_shift(h->cfg); const size_t S = (size_t)1 << sh;
    std::vector<ft8rx_record> r0((size_t)B * S);
    memset(r0.data(), 0, sizeof(ft8rx_record) * r0.size());
    std::vector<int32_t> nc(B, 0), where(n);
    for (int i = 0; i < n; i++) {
        if (frame[i] < 0 || frame[i] >= B || f0_idx[i] < -32768 || f0_idx[i] > 32767 || h0_idx[i] < -32768 || h0_idx[i] > 32767 ||
            ttweak[i] < -128 || ttweak[i] > 127 || ftweak[i] < -128 || ftweak[i] > 127) {
            set_err(h, "ft8rx_report_probe: candidate %d (frame %d, f0 %d, h0 %d, tweaks %d / %d) is out of range", i, frame[i], f0_idx[i], h0_idx[i], ttweak[i], ftweak[i]); return -1; }
        if (nc[frame[i]] >= (int)S) { set_err(h, "ft8rx_report_probe: more than %zu candidates in frame %d", S, frame[i]); return -1; }
        where[i] = (int32_t)((size_t)frame[i] * S + nc[frame[i]]++);
        ft8rx_record& r = r0[where[i]];
        r.msg_lo = msg_lo[i]; r.msg_hi = msg_hi[i]; r.f0_idx = (int16_t)f0_idx[i]; r.h0_idx = (int16_t)h0_idx[i];
        r.ttweak = (int8_t)ttweak[i]; r.ftweak = (int8_t)ftweak[i]; r.status = FT8RX_ST_DECODED;
    }
    ENTER(h);
    HIPCHK(h, hipMemcpy(h->d_spec, spec, sizeof(cpx) * (size_t)B * FT8RX_SPEC_BINS, hipMemcpyHostToDevice));
    Scratch Sc{h};
    ft8rx_record* d_rec = Sc.put(r0.data(), r0.size()); NEED(d_rec);
    int32_t* d_nc = Sc.put(nc.data(), nc.size()); NEED(d_nc);
    int32_t* d_items = Sc.get<int32_t>((size_t)B * S); NEED(d_items);
    int32_t* d_count = Sc.get<int32_t>(1); NEED(d_count);
    ft8rx_report* d_rep = Sc.get<ft8rx_report>((size_t)B * S); NEED(d_rep);
    launch_reports(h, B, h->d_spec, d_rec, d_nc, d_items, d_count, d_rep, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<ft8rx_report> out((size_t)B * S);
    HIPCHK(h, hipMemcpy(out.data(), d_rep, sizeof(ft8rx_report) * out.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) reports[i] = out[where[i]];
    return 0;
}

int ft8rx_osd_ext(ft8rx_handle* h, const float* llr, int n, int singleflips, int doubleflips, int tripleflips, int max_hd,
                  int32_t* ok, uint64_t* msg_lo, uint64_t* msg_hi, int32_t* trial, int32_t* hd) {
    if (!h || !llr || n < 1) return -1;
    if (singleflips < 0 || singleflips > OSD_MAXFLIP || doubleflips < 0 || doubleflips > OSD_MAXFLIP || tripleflips < 0 || tripleflips > 40 ||
        max_hd < 0 || max_hd > 174) { set_err(h, "ft8rx_osd: flip counts out of range"); return -1; }
    const std::vector<uint32_t> tr = osd_trial_table(singleflips, doubleflips, tripleflips);
    if (tr.size() > OSD_MAXTRIALS) { set_err(h, "ft8rx_osd: %zu trials exceed %d", tr.size(), OSD_MAXTRIALS); return -1; }
    ENTER(h);
    Scratch S{h};
    float* d_in = S.put(llr, (size_t)n * 174); NEED(d_in);
    uint32_t* d_tr = S.put(tr.data(), tr.size()); NEED(d_tr);
    Att* d_att = S.get<Att>(n); NEED(d_att);
    int32_t* d_nan = S.get<int32_t>((size_t)n + 1); NEED(d_nan);            // [0] = length of the list of NaN vectors, then the list
    HIPCHK(h, hipMemsetAsync(d_nan, 0, sizeof(int32_t), h->stream));
    const WorkList nanl{d_nan + 1, d_nan};
    launch_osd(h, 0, n, h->stream, 2, d_in, nullptr, nullptr, nullptr, nullptr, d_att, nullptr, nullptr, d_tr, (int)tr.size(),
               osd_nflip(singleflips, tripleflips), max_hd, cand_shift(h->cfg), WorkList{nullptr, nullptr}, nanl);      // (msg_types do not apply here)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<Att> a(n);
    HIPCHK(h, hipMemcpy(a.data(), d_att, sizeof(Att) * n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
        ok[i] = a[i].ok; msg_lo[i] = a[i].lo; msg_hi[i] = a[i].hi; trial[i] = a[i].ok ? a[i].n_its : -1;
        if (hd) hd[i] = a[i].ok ? a[i].pad[0] : -1;
    }
    return 0;
}

int ft8rx_osd(ft8rx_handle* h, const float* llr, int n, int singleflips, int doubleflips, int32_t* ok, uint64_t* msg_lo,
              uint64_t* msg_hi, int32_t* trial) {
    return ft8rx_osd_ext(h, llr, n, singleflips, doubleflips, 0, 0, ok, msg_lo, msg_hi, trial, nullptr);
}

int ft8rx_crc_valid(ft8rx_handle* h, const float* cw91, int n, int32_t* res, uint64_t* msg_lo, uint64_t* msg_hi) {
    if (!h || !cw91 || n < 1) return -1;
    ENTER(h);
    Scratch S{h};
    float* d_in = S.put(cw91, (size_t)n * 91); NEED(d_in);
    int32_t* d_res = S.get<int32_t>(n); NEED(d_res);
    uint64_t* d_lo = S.get<uint64_t>(n); NEED(d_lo);
    uint64_t* d_hi = S.get<uint64_t>(n); NEED(d_hi);
    k_crc_probe<<<n, 64, 0, h->stream>>>(d_in, n, d_res, d_lo, d_hi);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(res, d_res, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(msg_lo, d_lo, sizeof(uint64_t) * n, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(msg_hi, d_hi, sizeof(uint64_t) * n, hipMemcpyDeviceToHost));
    return 0;
}

int ft8rx_valid77(ft8rx_handle* h, const uint64_t* msg_lo, const uint64_t* msg_hi, int n, int32_t* valid) {
    if (!h || !msg_lo || !msg_hi || n < 1) return -1;
    ENTER(h);
    Scratch S{h};
    uint64_t* d_lo = S.put(msg_lo, n); NEED(d_lo);
    uint64_t* d_hi = S.put(msg_hi, n); NEED(d_hi);
    int32_t* d_v = S.get<int32_t>(n); NEED(d_v);
    k_valid_probe<<<(n + 255) / 256, 256, 0, h->stream>>>(d_lo, d_hi, n, d_v);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(valid, d_v, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return 0;
}

int ft8rx_valid77_ext(ft8rx_handle* h, const uint64_t* msg_lo, const uint64_t* msg_hi, int n, int32_t mask, int32_t* valid) {
    if (!h || !msg_lo || !msg_hi || n < 1 || mask < 0 || mask > FT8RX_MT_ALL) return -1;
    ENTER(h);
    Scratch S{h};
    uint64_t* d_lo = S.put(msg_lo, n); NEED(d_lo);
    uint64_t* d_hi = S.put(msg_hi, n); NEED(d_hi);
    int32_t* d_v = S.get<int32_t>(n); NEED(d_v);
    k_valid_ext_probe<<<(n + 255) / 256, 256, 0, h->stream>>>(d_lo, d_hi, n, (unsigned)mask, d_v);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(valid, d_v, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------------------- FT4 (kernels/ft4.hpp)
// Everything FT4 owns, at the first FT4 call on the handle, all or nothing (FirstUse)
static int ft4_workspaces(ft8rx_handle* h) {
    if (ws_ready(h, WS_FT4)) return 0;
    ft8rx_handle::Ft4& w = h->ft4;
    const size_t mf = (size_t)h->max_frames, S = mf << cand_shift(h->cfg);
    FirstUse F(h, WS_FT4);
    size_t bytes = 0;
    auto dev = [&](auto** p, size_t n) { F.dev(p, n); bytes += n * sizeof(**p); };
    dev(&w.d_audio, mf * FT8RX_FT4_NSAMP); dev(&w.d_grid, mf * FT8RX_FT4_ROWS * FT8RX_FT4_COLS);
    dev(&w.d_win, (size_t)FT4_NFFT); dev(&w.d_w576, (size_t)576); dev(&w.d_wr, (size_t)FT8RX_FT4_COLS);
    dev(&w.d_raw, mf * NF0MAX); dev(&w.d_kept, mf * NF0MAX); dev(&w.d_bh, mf * NF0MAX);
    dev(&w.d_trip, S * 3); dev(&w.d_llr, S * 174); dev(&w.d_saved, S * 174); dev(&w.d_tweak, S * 2); dev(&w.d_metric, S); dev(&w.d_snr, S);
    dev(&w.d_att, S); dev(&w.d_attO, S); dev(&w.d_items, S); dev(&w.d_dense, S * 174); dev(&w.d_nan, S + 1); dev(&w.d_count, (size_t)2);
    F.host(&w.h_count, (size_t)2);
    if (!F.rc) {
        std::vector<float> win(FT4_NFFT);
        for (int i = 0; i < FT4_NFFT; i++) win[i] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)i / (double)FT4_NFFT));
        std::vector<cpx> w576, wr;
        host_twiddle(576, 576, w576); host_twiddle(FT4_NFFT, FT8RX_FT4_COLS, wr);
        FIRST_HIP(F, hipMemcpy(w.d_win, win.data(), sizeof(float) * win.size(), hipMemcpyHostToDevice));
        FIRST_HIP(F, hipMemcpy(w.d_w576, w576.data(), sizeof(cpx) * w576.size(), hipMemcpyHostToDevice));
        FIRST_HIP(F, hipMemcpy(w.d_wr, wr.data(), sizeof(cpx) * wr.size(), hipMemcpyHostToDevice));
        FIRST_HIP(F, hipMemset(w.d_tweak, 0, sizeof(int32_t) * S * 2));
        FIRST_HIP(F, hipMemset(w.d_metric, 0, sizeof(float) * S));
        FIRST_HIP(F, hipMemset(w.d_snr, 0, sizeof(int32_t) * S));
    }
    const int rc = F.done();
    w.bytes = rc ? 0 : bytes;
    return rc;
}
// Everything the coherent step owns, at the first FT4 batch that runs with ft8rx_ft4_set_coherent on, all or nothing
static int ft4coh_workspaces(ft8rx_handle* h) {
    if (ws_ready(h, WS_FT4_COH)) return 0;
    ft8rx_handle::Ft4Coh& w = h->ft4coh;
    const size_t S = (size_t)h->max_frames << cand_shift(h->cfg);
    FirstUse F(h, WS_FT4_COH);
    size_t bytes = 0;
    auto dev = [&](auto** p, size_t n) { F.dev(p, n); bytes += n * sizeof(**p); };
    dev(&w.d_q, S); dev(&w.d_met, S * FT4_COH_NQ); dev(&w.d_llr, 2 * S * 174); dev(&w.d_saved, 2 * S * 174); dev(&w.d_att, 2 * S);
    dev(&w.d_items, S); dev(&w.d_count, (size_t)1);
    F.host(&w.h_count, (size_t)1);
    const int rc = F.done();
    w.bytes = rc ? 0 : bytes;
    return rc;
}
// Everything the weak search owns, at the first FT4 batch that runs with ft8rx_ft4_set_weak on, all or nothing.  The tables are filled
// from exact arguments: j n / 4608 and k / 32 of a turn
static int ft4weak_workspaces(ft8rx_handle* h) {
    if (ws_ready(h, WS_FT4_WEAK)) return 0;
    ft8rx_handle::Ft4Weak& w = h->ft4weak;
    FirstUse F(h, WS_FT4_WEAK);
    size_t bytes = 0;
    auto dev = [&](auto** p, size_t n) { F.dev(p, n); bytes += n * sizeof(**p); };
    dev(&w.d_cg, (size_t)h->max_frames * FT4W_ROWS * FT4W_NFQ); dev(&w.d_mix, (size_t)FT4W_NMIX * 576); dev(&w.d_rot, (size_t)32);
    if (!F.rc) {
        std::vector<cpx> mix((size_t)FT4W_NMIX * 576), rot;
        for (int j = 0; j < FT4W_NMIX; j++) for (int n = 0; n < 576; n++) {
            const double ang = 2.0 * M_PI * (double)((j * n) % 4608) / 4608.0;
            mix[(size_t)j * 576 + n] = make_float2((float)cos(ang), (float)(-sin(ang)));
        }
        host_twiddle(32, 32, rot);
        FIRST_HIP(F, hipMemcpy(w.d_mix, mix.data(), sizeof(cpx) * mix.size(), hipMemcpyHostToDevice));
        FIRST_HIP(F, hipMemcpy(w.d_rot, rot.data(), sizeof(cpx) * rot.size(), hipMemcpyHostToDevice));
    }
    const int rc = F.done();
    w.bytes = rc ? 0 : bytes;
    return rc;
}
// Everything OSD on the coherent rows owns, at the first FT4 batch that runs with ft8rx_ft4_set_coh_osd and the coherent step on, all
// or nothing
static int ft4cosd_workspaces(ft8rx_handle* h) {
    if (ws_ready(h, WS_FT4_COSD)) return 0;
    ft8rx_handle::Ft4Cosd& w = h->ft4cosd;
    const size_t S = (size_t)h->max_frames << cand_shift(h->cfg);
    FirstUse F(h, WS_FT4_COSD);
    size_t bytes = 0;
    auto dev = [&](auto** p, size_t n) { F.dev(p, n); bytes += n * sizeof(**p); };
    dev(&w.d_pos, S); dev(&w.d_dense, 2 * S * 174); dev(&w.d_att, 2 * S); dev(&w.d_nan, 2 * S + 1); dev(&w.d_score, 2 * S);
    const int rc = F.done();
    w.bytes = rc ? 0 : bytes;
    return rc;
}
static int ft4_refuse(ft8rx_handle* h, const char* who) {
    const int c = optins::conflict(active_optins(h), optins::FT4_ROW);
    if (c < 0) return 0;
    set_err(h, "%s: %s is not supported together with %s", who, optins::FT4_ROW.name, optins::TABLE[c].name);
    return -1;
}
static void ft4_launch_grid(ft8rx_handle* h, const int16_t* d_audio, int B, float* grid, float* power, hipStream_t s) {
    k_ft4_grid<<<dim3(FT8RX_FT4_ROWS / FT4_GR, B), FT4_GRID_NT, 0, s>>>(d_audio, grid, power, h->ft4.d_win, h->ft4.d_w576, h->ft4.d_wr);
}
// the per-f0 maxima (d_raw, d_bh) -> the survivors at or above `floor` (d_kept), then k_topk's records and counts
static void ft4_launch_peaks(ft8rx_handle* h, int B, float floor, ft8rx_record* rec, int32_t* ncand, int32_t* evcount, hipStream_t s) {
    const ft8rx_handle::Ft4& w = h->ft4;
    const int nf0 = w.range.f0_hi - w.range.f0_lo;
    k_ft4_peaks<<<dim3((nf0 + 255) / 256, B), 256, 0, s>>>(w.d_raw, w.d_kept, nf0, floor, B);
    ft8rx_config c = h->cfg;
    c.f0_lo = w.range.f0_lo; c.f0_hi = w.range.f0_hi; c.sync_score_min = 0.0f;      // k_topk: every surviving (positive) score, best first
    k_topk<<<B, 1024, 0, s>>>(w.d_kept, w.d_bh, rec, ncand, c, evcount, nullptr, nullptr);
}
// grid -> the per-f0 maxima, then ft4_launch_peaks
static void ft4_launch_sync(ft8rx_handle* h, const float* grid, int B, ft8rx_record* rec, int32_t* ncand, int32_t* evcount, hipStream_t s) {
    const ft8rx_handle::Ft4& w = h->ft4;
    const int nf0 = w.range.f0_hi - w.range.f0_lo;
    k_ft4_sync<<<dim3((nf0 + 15) / 16, B), 256, 0, s>>>(grid, w.d_raw, w.d_bh, w.range);
    ft4_launch_peaks(h, B, w.sync_min, rec, ncand, evcount, s);
}
// the weak search (section 19.10): the complex grid on the rows the h0 range reads, those with a sample inside the frame ...
static void ft4_launch_cgrid(ft8rx_handle* h, const int16_t* d_audio, int B, hipStream_t s) {
    const ft8rx_handle::Ft4Weak& k = h->ft4weak;
    const int lo = std::max(h->ft4.range.h0_lo + 4, FT4W_ROW_LO), hi = std::min(h->ft4.range.h0_hi + 4 * (FT4_NSYM - 2), FT4W_ROW_LO + FT4W_ROWS);
    if (hi > lo) k_ft4_cgrid<<<dim3((hi - lo + FT4W_CR - 1) / FT4W_CR, B), FT4W_NT, 0, s>>>(d_audio, k.d_cg, k.d_mix, k.d_rot, h->ft4.d_w576, lo, hi);
}
// ... and its per-f0 maxima where k_ft4_sync writes its own, cut at weak_min
static void ft4_launch_csync(ft8rx_handle* h, int B, ft8rx_record* rec, int32_t* ncand, int32_t* evcount, hipStream_t s) {
    const ft8rx_handle::Ft4& w = h->ft4;
    const int nf0 = w.range.f0_hi - w.range.f0_lo;
    k_ft4_csync<<<dim3((nf0 + 15) / 16, B), 256, 0, s>>>(h->ft4weak.d_cg, w.d_raw, w.d_bh, w.range);
    ft4_launch_peaks(h, B, h->ft4weak.weak_min, rec, ncand, evcount, s);
}
// BP then OSD on n raw LLR vectors with the FT4 flag; att / attO [n]; OSD runs on every vector (the stage entries) -- the chain calls
// the two halves itself.  mt: FT8RX_MT_* bits
static void ft4_launch_bp(ft8rx_handle* h, const float* llr, int n, int nc0, int iters, unsigned mt, Att* att, float* saved, hipStream_t s) {
    k_bp_ext<<<n, 64, 0, s>>>(2, llr, nullptr, nullptr, nullptr, att, saved, nullptr, nullptr, h->cfg, nc0, iters, WorkList{nullptr, nullptr}, 0, 1, mt | FT8_MT_FT4);
}
static void ft4_launch_osd(ft8rx_handle* h, const float* llr, int n, const uint32_t* trials, int ntr, int nflip, int max_hd, unsigned mt, Att* attO,
                           int32_t* nan /*[n + 1], [0] zeroed*/, hipStream_t s) {
    launch_osd(h, mt | FT8_MT_FT4, n, s, 2, llr, nullptr, nullptr, nullptr, nullptr, attO, nullptr, nullptr, trials, ntr, nflip, max_hd,
               cand_shift(h->cfg), WorkList{nullptr, nullptr}, WorkList{nan + 1, nan});
}

// One FT4 batch on the main stream into the next result slot: grid, search, demodulation, BP, the OSD list (one host round trip for
// its length: OSD's raw-vector mode takes one block per vector), OSD, records and events; then the FT8 result tail (batch_finish).
// With ft8rx_ft4_set_coherent on, the coherent step stands between the list and OSD and shortens the list.
// With ft8rx_ft4_set_weak on, the complex grid and the coherent score stand in for grid and search (section 19.10); the rest is the same.
static int ft4_launch_batch(ft8rx_handle* h, const char* who, const int16_t* audio, bool on_host, int B) {
    HIPCHK(h, hipSetDevice(h->device));
    if (ft4_refuse(h, who)) return -1;
    if (const int rc = ft4_workspaces(h)) return rc;
    const bool coh = h->ft4coh.on;
    if (coh) if (const int rc = ft4coh_workspaces(h)) return rc;
    const bool weak = h->ft4weak.on;
    if (weak) if (const int rc = ft4weak_workspaces(h)) return rc;
    const bool cosd = coh && h->ft4cosd.on;
    if (cosd) if (const int rc = ft4cosd_workspaces(h)) return rc;
    ft8rx_handle::Ft4& w = h->ft4;
    const int slot = h->slot_enq;
    ResultSlot& sl = h->slots[slot];
    h->pnames.clear();
    if (h->inflight == 2) { h->slot_fetch ^= 1; h->inflight = 1; }          // the oldest unfetched batch is dropped
    sl.recall = false; sl.reports = false;
    { const int q = quiesce(h, true); if (q) return q; }
    hipStream_t s = h->stream;
    HIPCHK(h, hipStreamWaitEvent(s, sl.ev_done, 0));                        // the slot's previous results have left the device
    const int16_t* d_audio = audio;
    if (on_host) {
        HIPCHK(h, hipMemcpyAsync(w.d_audio, audio, sizeof(int16_t) * (size_t)B * FT8RX_FT4_NSAMP, hipMemcpyHostToDevice, s));
        d_audio = w.d_audio;
    }
    const ft8rx_config& c = h->cfg;
    const int sh = cand_shift(c), n = B << sh;
    const unsigned mt = (unsigned)h->msg_types;
    const bool prof = h->profiling;
#define STAGE(name) do { if (prof) { hipEventRecord(h->pev[h->pnames.size()], s); h->pnames.push_back(name); } } while (0)
    if (weak) {                                                             // section 19.10: in place of the dB grid and its search
        STAGE("ft4_cgrid");
        ft4_launch_cgrid(h, d_audio, B, s);
        STAGE("ft4_csync");
        ft4_launch_csync(h, B, sl.rec, sl.ncand, sl.evcount, s);
    } else {
        STAGE("ft4_grid");
        ft4_launch_grid(h, d_audio, B, w.d_grid, nullptr, s);
        STAGE("ft4_sync");
        ft4_launch_sync(h, w.d_grid, B, sl.rec, sl.ncand, sl.evcount, s);
    }
    STAGE("ft4_demod");
    k_ft4_trip<<<(n + 255) / 256, 256, 0, s>>>(sl.rec, sl.ncand, B, sh, w.d_trip);
    k_ft4_demod<<<n, FT4_DEMOD_NT, 0, s>>>(d_audio, w.d_trip, w.d_llr, w.d_tweak, w.d_metric, w.d_snr);
    STAGE("ft4_bp");
    ft4_launch_bp(h, w.d_llr, n, c.bp_nc0_b, c.bp_iters_b, mt, w.d_att, w.d_saved, s);
    HIPCHK(h, hipMemsetAsync(w.d_count, 0, 2 * sizeof(int32_t), s));
    k_ft4_after_bp<<<(n + 255) / 256, 256, 0, s>>>(sl.rec, sl.ncand, B, sh, w.d_att, w.d_tweak, w.d_snr, sl.ev, sl.evcount, WorkList{w.d_items, w.d_count});
    HIPCHK(h, hipMemcpyAsync(w.h_count, w.d_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    int n_osd = w.h_count[0];
    if (n_osd < 0 || n_osd > n) { set_err(h, "%s: the OSD list holds %d of %d slots", who, n_osd, n); return -2; }
    const int32_t* osd_items = w.d_items;
    const int n_coh = coh ? n_osd : 0;                                      // the rows k_ft4_coh fills, indexed by the first list
    if (coh && n_osd > 0) {
        // the coherent step on the failure list: run-of-2 and run-of-4 LLRs, the same BP on both rows in one launch (run length 2
        // wins), and what neither decodes goes on to OSD in list order -- a second read-back, of the shorter list's length
        STAGE("ft4_coh");
        const ft8rx_handle::Ft4Coh& k = h->ft4coh;
        const int nl = n_osd;
        k_ft4_coh<<<nl, FT4_DEMOD_NT, 0, s>>>(d_audio, w.d_trip, w.d_tweak, w.d_items, k.d_q, k.d_met, k.d_llr, k.d_llr + (size_t)nl * 174);
        ft4_launch_bp(h, k.d_llr, 2 * nl, c.bp_nc0_b, c.bp_iters_b, mt, k.d_att, k.d_saved, s);
        HIPCHK(h, hipMemsetAsync(k.d_count, 0, sizeof(int32_t), s));
        k_ft4_after_coh<<<(nl + 255) / 256, 256, 0, s>>>(sl.rec, sh, k.d_att, w.d_items, nl, sl.ev, sl.evcount, WorkList{k.d_items, k.d_count});
        HIPCHK(h, hipMemcpyAsync(k.h_count, k.d_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        n_osd = k.h_count[0];
        if (n_osd < 0 || n_osd > nl) { set_err(h, "%s: the OSD list behind the coherent step holds %d of %d items", who, n_osd, nl); return -2; }
        osd_items = k.d_items;
    }
    STAGE("ft4_osd");
    if (n_osd > 0) {
        k_ft4_gather<<<n_osd, 64, 0, s>>>(w.d_llr, osd_items, w.d_dense);
        HIPCHK(h, hipMemsetAsync(w.d_nan, 0, sizeof(int32_t), s));
        ft4_launch_osd(h, w.d_dense, n_osd, h->d_trials, h->n_trials, osd_nflip(c.osd_single, c.osd_triple), w.osd_max_hd, mt, w.d_attO, w.d_nan, s);
        k_ft4_after_osd<<<(n_osd + 255) / 256, 256, 0, s>>>(sl.rec, sh, w.d_attO, osd_items, n_osd, sl.ev, sl.evcount);
    }
    if (cosd && n_osd > 0) {
        // section 19.11: OSD once more, on the run-of-2 and then the run-of-4 rows of every item of its list (on all of them, not only the
        // exhausted ones: no third read-back), under the wide gate; the score of each returned word; then what a candidate left
        // EXHAUSTED may take
        STAGE("ft4_cosd");
        const ft8rx_handle::Ft4Cosd& v = h->ft4cosd;
        const ft8rx_handle::Ft4Coh& k = h->ft4coh;
        k_ft4_cosd_pos<<<(n_coh + 255) / 256, 256, 0, s>>>(w.d_items, n_coh, v.d_pos);
        k_ft4_cosd_gather<<<2 * n_osd, 64, 0, s>>>(k.d_llr, n_coh, osd_items, n_osd, v.d_pos, v.d_dense);
        HIPCHK(h, hipMemsetAsync(v.d_nan, 0, sizeof(int32_t), s));
        ft4_launch_osd(h, v.d_dense, 2 * n_osd, h->d_trials, h->n_trials, osd_nflip(c.osd_single, c.osd_triple), v.max_hd, mt, v.d_att, v.d_nan, s);
        k_ft4_verify<<<2 * n_osd, FT4_DEMOD_NT, 0, s>>>(d_audio, w.d_trip, w.d_tweak, osd_items, v.d_pos, k.d_q, v.d_att, sl.rec, n_osd, v.d_score, nullptr);
        k_ft4_after_cosd<<<(n_osd + 255) / 256, 256, 0, s>>>(sl.rec, sh, v.d_att, v.d_score, osd_items, n_osd, v.min_score, sl.ev, sl.evcount);
    }
    if (prof) hipEventRecord(h->pev[h->pnames.size()], s);
#undef STAGE
    HIPCHK(h, hipGetLastError());
    return batch_finish(h, slot, B, s);
}
static bool ft4_frames_ok(ft8rx_handle* h, const char* who, const void* audio, int B) {
    if (!h || !audio) return false;
    if (B < 1 || B > h->max_frames) { set_err(h, "%s: n_frames %d outside [1, %d]", who, B, h->max_frames); return false; }
    return true;
}

int ft8rx_ft4_enqueue_batch(ft8rx_handle* h, const int16_t* d_audio, int B) {
    if (!ft4_frames_ok(h, "ft8rx_ft4_enqueue_batch", d_audio, B)) return -1;
    if ((uintptr_t)d_audio % 4) { set_err(h, "ft8rx_ft4_enqueue_batch: d_audio is not aligned to 4 bytes (a pair of int16 samples)"); return -1; }
    return ft4_launch_batch(h, "ft8rx_ft4_enqueue_batch", d_audio, false, B);
}
int ft8rx_ft4_decode_batch(ft8rx_handle* h, const int16_t* audio, int B, ft8rx_record* records, int32_t* counts, ft8rx_event* events, int32_t* event_counts) {
    if (!ft4_frames_ok(h, "ft8rx_ft4_decode_batch", audio, B)) return -1;
    h->inflight = 0; h->slot_fetch = h->slot_enq;
    if (const int rc = ft4_launch_batch(h, "ft8rx_ft4_decode_batch", audio, true, B)) return rc;
    return ft8rx_fetch_results(h, B, records, counts, events, event_counts);
}
int ft8rx_ft4_decode_messages(ft8rx_handle* h, const int16_t* audio, int B, ft8rx_message* out, int max_msgs, int32_t* out_counts,
                              int n_threads, ft8rx_hashes* table, int32_t* flags) {
    if (!ft4_frames_ok(h, "ft8rx_ft4_decode_messages", audio, B) || !out || !out_counts) return -1;
    if (max_msgs < 1) { set_err(h, "ft8rx_ft4_decode_messages: bad max_msgs"); return -1; }
    if (h->msg_types) { set_err(h, "ft8rx_ft4_decode_messages: not supported together with msg_types != 0 (ft8rx_message rows cannot carry it); "
                                   "use ft8rx_ft4_decode_batch with ft8rx_package_batch_ext"); return -1; }
    h->inflight = 0; h->slot_fetch = h->slot_enq;
    int rc = ft4_launch_batch(h, "ft8rx_ft4_decode_messages", audio, true, B);
    if (rc) return rc;
    const ft8rx_record* rec; const int32_t* cnt; const ft8rx_event* ev; const int32_t* evc;
    rc = ft8rx_fetch_results_view(h, B, &rec, &cnt, &ev, &evc);
    if (rc) return rc;
    return hostmsg::package_batch(rec, cnt, ev, evc, B, h->cfg.max_cands, out, max_msgs, out_counts, n_threads, table ? &table->H : nullptr, flags);
}

int ft8rx_ft4_set(ft8rx_handle* h, float sync_min, int32_t osd_max_hd) {
    if (!h) return -1;
    if (sync_min == 0.0f) sync_min = FT8RX_FT4_SYNC_MIN_DEFAULT;
    if (osd_max_hd == 0) osd_max_hd = FT8RX_FT4_OSD_MAX_HD_DEFAULT;
    if (!(sync_min > 0.0f) || !(sync_min < INFINITY)) { set_err(h, "ft8rx_ft4_set: sync_min %g must be a positive score (0 = the default)", (double)sync_min); return -1; }
    if (osd_max_hd < 1 || osd_max_hd > 174) { set_err(h, "ft8rx_ft4_set: osd_max_hd %d outside [1, 174] (0 = the default)", osd_max_hd); return -1; }
    h->ft4.sync_min = sync_min; h->ft4.osd_max_hd = osd_max_hd;
    return 0;
}
int ft8rx_ft4_set_range(ft8rx_handle* h, int32_t f0_lo, int32_t f0_hi, int32_t h0_lo, int32_t h0_hi) {
    if (!h) return -1;
    if (!f0_lo && !f0_hi && !h0_lo && !h0_hi) { h->ft4.range = ft8rx_handle::Ft4().range; return 0; }
    if (f0_lo < 0 || f0_hi <= f0_lo || f0_hi > FT8RX_FT4_COLS - 6 || h0_lo < -1024 || h0_hi <= h0_lo || h0_hi > 1024) {
        set_err(h, "ft8rx_ft4_set_range: bins [%d, %d) must lie in [0, %d), rows [%d, %d) in [-1024, 1024)", f0_lo, f0_hi, FT8RX_FT4_COLS - 6, h0_lo, h0_hi); return -1; }
    h->ft4.range = Ft4Range{f0_lo, f0_hi, h0_lo, h0_hi};
    return 0;
}
int ft8rx_ft4_info(ft8rx_handle* h, uint64_t* workspace_bytes, float* sync_min, int32_t* osd_max_hd, int32_t* range) {
    if (!h) return -1;
    if (workspace_bytes) *workspace_bytes = ws_ready(h, WS_FT4) ? (uint64_t)h->ft4.bytes : 0;
    if (sync_min) *sync_min = h->ft4.sync_min;
    if (osd_max_hd) *osd_max_hd = h->ft4.osd_max_hd;
    if (range) { range[0] = h->ft4.range.f0_lo; range[1] = h->ft4.range.f0_hi; range[2] = h->ft4.range.h0_lo; range[3] = h->ft4.range.h0_hi; }
    return 0;
}

int ft8rx_ft4_set_coherent(ft8rx_handle* h, int32_t on) {
    if (!h) return -1;
    h->ft4coh.on = on != 0;
    return 0;
}
int ft8rx_ft4_coh_info(ft8rx_handle* h, uint64_t* workspace_bytes, int32_t* on) {
    if (!h) return -1;
    if (workspace_bytes) *workspace_bytes = ws_ready(h, WS_FT4_COH) ? (uint64_t)h->ft4coh.bytes : 0;
    if (on) *on = h->ft4coh.on ? 1 : 0;
    return 0;
}

int ft8rx_ft4_set_weak(ft8rx_handle* h, int32_t on, float weak_min) {
    if (!h) return -1;
    h->ft4weak.on = on != 0;
    h->ft4weak.weak_min = (weak_min > 0.0f && weak_min < INFINITY) ? weak_min : FT8RX_FT4_WEAK_MIN_DEFAULT;
    return 0;
}
int ft8rx_ft4_weak_info(ft8rx_handle* h, uint64_t* workspace_bytes, int32_t* on, float* weak_min) {
    if (!h) return -1;
    if (workspace_bytes) *workspace_bytes = ws_ready(h, WS_FT4_WEAK) ? (uint64_t)h->ft4weak.bytes : 0;
    if (on) *on = h->ft4weak.on ? 1 : 0;
    if (weak_min) *weak_min = h->ft4weak.weak_min;
    return 0;
}
// ---- OSD on the coherent rows (kernels/ft4_verify.hpp)
int ft8rx_ft4_set_coh_osd(ft8rx_handle* h, int32_t on, float min_score, int32_t max_hd) {
    if (!h) return -1;
    h->ft4cosd.on = on != 0;
    h->ft4cosd.min_score = (min_score > 0.0f && min_score < INFINITY) ? min_score : FT8RX_FT4_COH_OSD_MIN_SCORE_DEFAULT;
    h->ft4cosd.max_hd = max_hd <= 0 ? FT8RX_FT4_COH_OSD_MAX_HD_DEFAULT : max_hd > 174 ? 174 : max_hd;
    return 0;
}
int ft8rx_ft4_coh_osd_info(ft8rx_handle* h, uint64_t* workspace_bytes, int32_t* on, float* min_score, int32_t* max_hd) {
    if (!h) return -1;
    if (workspace_bytes) *workspace_bytes = ws_ready(h, WS_FT4_COSD) ? (uint64_t)h->ft4cosd.bytes : 0;
    if (on) *on = h->ft4cosd.on ? 1 : 0;
    if (min_score) *min_score = h->ft4cosd.min_score;
    if (max_hd) *max_hd = h->ft4cosd.max_hd;
    return 0;
}

int ft8rx_ft4_grid(ft8rx_handle* h, const int16_t* audio, int B, float* grid, float* power) {
    if (!ft4_frames_ok(h, "ft8rx_ft4_grid", audio, B) || !grid) return -1;
    ENTER(h);
    if (const int rc = ft4_workspaces(h)) return rc;
    ft8rx_handle::Ft4& w = h->ft4;
    const size_t n = (size_t)B * FT8RX_FT4_ROWS * FT8RX_FT4_COLS;
    Scratch S{h};
    float* d_pw = nullptr;
    if (power) { d_pw = S.get<float>(n); NEED(d_pw); }
    HIPCHK(h, hipMemcpy(w.d_audio, audio, sizeof(int16_t) * (size_t)B * FT8RX_FT4_NSAMP, hipMemcpyHostToDevice));
    ft4_launch_grid(h, w.d_audio, B, w.d_grid, d_pw, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(grid, w.d_grid, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (power) HIPCHK(h, hipMemcpy(power, d_pw, sizeof(float) * n, hipMemcpyDeviceToHost));
    return 0;
}
// the read-back of the search's stage entries: the records' (f0, h0, score) in output order, the counts, the per-bin maxima
static int ft4_sync_results(ft8rx_handle* h, int B, int32_t* f0_idx, int32_t* h0_idx, float* score, int32_t* counts, float* best_score, int32_t* best_h0) {
    ft8rx_handle::Ft4& w = h->ft4;
    const int sh = cand_shift(h->cfg), mc = h->cfg.max_cands, nf0 = w.range.f0_hi - w.range.f0_lo;
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<ft8rx_record> rec((size_t)B << sh);
    HIPCHK(h, hipMemcpy(rec.data(), h->d_rec, sizeof(ft8rx_record) * rec.size(), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(counts, h->d_ncand, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    for (int f = 0; f < B; f++) for (int i = 0; i < mc; i++) {
        const ft8rx_record& r = rec[((size_t)f << sh) + i];
        const bool live = i < counts[f];
        f0_idx[(size_t)f * mc + i] = live ? r.f0_idx : 0; h0_idx[(size_t)f * mc + i] = live ? r.h0_idx : 0; score[(size_t)f * mc + i] = live ? r.score : 0.0f;
    }
    if (best_score) HIPCHK(h, hipMemcpy2D(best_score, sizeof(float) * nf0, w.d_raw, sizeof(float) * NF0MAX, sizeof(float) * nf0, B, hipMemcpyDeviceToHost));
    if (best_h0) HIPCHK(h, hipMemcpy2D(best_h0, sizeof(int32_t) * nf0, w.d_bh, sizeof(int32_t) * NF0MAX, sizeof(int32_t) * nf0, B, hipMemcpyDeviceToHost));
    return 0;
}
int ft8rx_ft4_sync(ft8rx_handle* h, const float* grid, int B, int32_t* f0_idx, int32_t* h0_idx, float* score, int32_t* counts,
                   float* best_score, int32_t* best_h0) {
    if (!ft4_frames_ok(h, "ft8rx_ft4_sync", grid, B) || !f0_idx || !h0_idx || !score || !counts) return -1;
    ENTER(h);
    if (const int rc = ft4_workspaces(h)) return rc;
    ft8rx_handle::Ft4& w = h->ft4;
    HIPCHK(h, hipMemcpy(w.d_grid, grid, sizeof(float) * (size_t)B * FT8RX_FT4_ROWS * FT8RX_FT4_COLS, hipMemcpyHostToDevice));
    ft4_launch_sync(h, w.d_grid, B, h->d_rec, h->d_ncand, h->d_evcount, h->stream);
    return ft4_sync_results(h, B, f0_idx, h0_idx, score, counts, best_score, best_h0);
}
int ft8rx_ft4_sync_weak(ft8rx_handle* h, const int16_t* audio, int B, int32_t* f0_idx, int32_t* h0_idx, float* score, int32_t* counts,
                        float* best_score, int32_t* best_h0) {
    if (!ft4_frames_ok(h, "ft8rx_ft4_sync_weak", audio, B) || !f0_idx || !h0_idx || !score || !counts) return -1;
    ENTER(h);
    if (const int rc = ft4_workspaces(h)) return rc;
    if (const int rc = ft4weak_workspaces(h)) return rc;
    HIPCHK(h, hipMemcpy(h->ft4.d_audio, audio, sizeof(int16_t) * (size_t)B * FT8RX_FT4_NSAMP, hipMemcpyHostToDevice));
    ft4_launch_cgrid(h, h->ft4.d_audio, B, h->stream);
    ft4_launch_csync(h, B, h->d_rec, h->d_ncand, h->d_evcount, h->stream);
    return ft4_sync_results(h, B, f0_idx, h0_idx, score, counts, best_score, best_h0);
}
int ft8rx_ft4_demod(ft8rx_handle* h, const int16_t* audio, int B, int n, const int32_t* frame, const int32_t* f0_idx, const int32_t* h0_idx,
                    int32_t* tweak, float* metric, float* llr, int32_t* snr) {
    if (!ft4_frames_ok(h, "ft8rx_ft4_demod", audio, B) || n < 1 || !frame || !f0_idx || !h0_idx || !tweak || !metric || !llr || !snr) return -1;
    for (int i = 0; i < n; i++)
        if (frame[i] < 0 || frame[i] >= B || f0_idx[i] < 0 || f0_idx[i] >= FT8RX_FT4_COLS - 6 || h0_idx[i] < -1024 || h0_idx[i] >= 1024) {
            set_err(h, "ft8rx_ft4_demod: candidate %d (frame %d, f0 %d, h0 %d) is out of range", i, frame[i], f0_idx[i], h0_idx[i]); return -1; }
    ENTER(h);
    if (const int rc = ft4_workspaces(h)) return rc;
    ft8rx_handle::Ft4& w = h->ft4;
    const std::vector<int32_t> trip = pack_triples(n, frame, f0_idx, h0_idx);
    Scratch S{h};
    int32_t* d_trip = S.put(trip.data(), trip.size()); NEED(d_trip);
    float* d_llr = S.get<float>((size_t)n * 174); NEED(d_llr);
    int32_t* d_tw = S.get<int32_t>((size_t)n * 2); NEED(d_tw);
    float* d_met = S.get<float>(n); NEED(d_met);
    int32_t* d_snr = S.get<int32_t>(n); NEED(d_snr);
    HIPCHK(h, hipMemcpy(w.d_audio, audio, sizeof(int16_t) * (size_t)B * FT8RX_FT4_NSAMP, hipMemcpyHostToDevice));
    k_ft4_demod<<<n, FT4_DEMOD_NT, 0, h->stream>>>(w.d_audio, d_trip, d_llr, d_tw, d_met, d_snr);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(llr, d_llr, sizeof(float) * (size_t)n * 174, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(tweak, d_tw, sizeof(int32_t) * (size_t)n * 2, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(metric, d_met, sizeof(float) * n, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(snr, d_snr, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return 0;
}
int ft8rx_ft4_coherent(ft8rx_handle* h, const int16_t* audio, int B, int n, const int32_t* frame, const int32_t* f0_idx, const int32_t* h0_idx,
                       const int32_t* ttweak, const int32_t* ftweak, int32_t* q, float* metrics, float* llr2, float* llr4) {
    if (!ft4_frames_ok(h, "ft8rx_ft4_coherent", audio, B) || n < 1 || !frame || !f0_idx || !h0_idx || !ttweak || !ftweak || !q || !metrics || !llr2 || !llr4) return -1;
    for (int i = 0; i < n; i++)
        if (frame[i] < 0 || frame[i] >= B || f0_idx[i] < 0 || f0_idx[i] >= FT8RX_FT4_COLS - 6 || h0_idx[i] < -1024 || h0_idx[i] >= 1024 ||
            ttweak[i] < -(FT4_N_DT / 2) || ttweak[i] > FT4_N_DT / 2 || ftweak[i] < -(FT4_N_DF / 2) || ftweak[i] > FT4_N_DF / 2) {
            set_err(h, "ft8rx_ft4_coherent: candidate %d (frame %d, f0 %d, h0 %d, tt %d, ft %d) is out of range", i, frame[i], f0_idx[i], h0_idx[i], ttweak[i], ftweak[i]);
            return -1; }
    ENTER(h);
    if (const int rc = ft4_workspaces(h)) return rc;
    ft8rx_handle::Ft4& w = h->ft4;
    const std::vector<int32_t> trip = pack_triples(n, frame, f0_idx, h0_idx);
    std::vector<int32_t> tw((size_t)n * 2);
    for (int i = 0; i < n; i++) { tw[2 * i] = ttweak[i]; tw[2 * i + 1] = ftweak[i]; }
    Scratch S{h};
    int32_t* d_trip = S.put(trip.data(), trip.size()); NEED(d_trip);
    int32_t* d_tw = S.put(tw.data(), tw.size()); NEED(d_tw);
    int32_t* d_q = S.get<int32_t>(n); NEED(d_q);
    float* d_met = S.get<float>((size_t)n * FT4_COH_NQ); NEED(d_met);
    float* d_l2 = S.get<float>((size_t)n * 174); NEED(d_l2);
    float* d_l4 = S.get<float>((size_t)n * 174); NEED(d_l4);
    HIPCHK(h, hipMemcpy(w.d_audio, audio, sizeof(int16_t) * (size_t)B * FT8RX_FT4_NSAMP, hipMemcpyHostToDevice));
    k_ft4_coh<<<n, FT4_DEMOD_NT, 0, h->stream>>>(w.d_audio, d_trip, d_tw, nullptr, d_q, d_met, d_l2, d_l4);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(q, d_q, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(metrics, d_met, sizeof(float) * (size_t)n * FT4_COH_NQ, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(llr2, d_l2, sizeof(float) * (size_t)n * 174, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(llr4, d_l4, sizeof(float) * (size_t)n * 174, hipMemcpyDeviceToHost));
    return 0;
}
int ft8rx_ft4_verify(ft8rx_handle* h, const int16_t* audio, int B, int n, const int32_t* frame, const int32_t* f0_idx, const int32_t* h0_idx,
                     const int32_t* ttweak, const int32_t* ftweak, const int32_t* q, const uint64_t* msg_lo, const uint64_t* msg_hi, float* score,
                     uint8_t* tones) {
    if (!ft4_frames_ok(h, "ft8rx_ft4_verify", audio, B) || n < 1 || !frame || !f0_idx || !h0_idx || !ttweak || !ftweak || !q || !msg_lo || !msg_hi || !score) return -1;
    for (int i = 0; i < n; i++)
        if (frame[i] < 0 || frame[i] >= B || f0_idx[i] < 0 || f0_idx[i] >= FT8RX_FT4_COLS - 6 || h0_idx[i] < -1024 || h0_idx[i] >= 1024 ||
            ttweak[i] < -(FT4_N_DT / 2) || ttweak[i] > FT4_N_DT / 2 || ftweak[i] < -(FT4_N_DF / 2) || ftweak[i] > FT4_N_DF / 2 || q[i] < -4 || q[i] > 4) {
            set_err(h, "ft8rx_ft4_verify: candidate %d (frame %d, f0 %d, h0 %d, tt %d, ft %d, q %d) is out of range", i, frame[i], f0_idx[i], h0_idx[i], ttweak[i], ftweak[i], q[i]);
            return -1; }
    ENTER(h);
    if (const int rc = ft4_workspaces(h)) return rc;
    ft8rx_handle::Ft4& w = h->ft4;
    const std::vector<int32_t> trip = pack_triples(n, frame, f0_idx, h0_idx);
    std::vector<int32_t> tw((size_t)n * 2);
    std::vector<Att> att(n);
    for (int i = 0; i < n; i++) {
        tw[2 * i] = ttweak[i]; tw[2 * i + 1] = ftweak[i];
        att[i] = Att{}; att[i].lo = msg_lo[i]; att[i].hi = msg_hi[i] & 0x1FFFull; att[i].ok = 1;
    }
    Scratch S{h};
    int32_t* d_trip = S.put(trip.data(), trip.size()); NEED(d_trip);
    int32_t* d_tw = S.put(tw.data(), tw.size()); NEED(d_tw);
    int32_t* d_q = S.put(q, (size_t)n); NEED(d_q);
    Att* d_att = S.put(att.data(), att.size()); NEED(d_att);
    float* d_sc = S.get<float>(n); NEED(d_sc);
    uint8_t* d_tn = nullptr;
    if (tones) { d_tn = S.get<uint8_t>((size_t)n * FT4_NSYM); NEED(d_tn); }
    HIPCHK(h, hipMemcpy(w.d_audio, audio, sizeof(int16_t) * (size_t)B * FT8RX_FT4_NSAMP, hipMemcpyHostToDevice));
    k_ft4_verify<<<n, FT4_DEMOD_NT, 0, h->stream>>>(w.d_audio, d_trip, d_tw, nullptr, nullptr, d_q, d_att, nullptr, n, d_sc, d_tn);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(score, d_sc, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (tones) HIPCHK(h, hipMemcpy(tones, d_tn, (size_t)n * FT4_NSYM, hipMemcpyDeviceToHost));
    return 0;
}
int ft8rx_ft4_ldpc(ft8rx_handle* h, const float* llr, int n, int max_ncheck0, int max_iters, int32_t mask, int32_t* ok, uint64_t* msg_lo,
                   uint64_t* msg_hi, int32_t* n_its, int32_t* has_out, float* llr_out) {
    if (!h || !llr || n < 1 || !ok || !msg_lo || !msg_hi || !n_its || !has_out) return -1;
    if (mask < 0 || mask > FT8RX_MT_ALL) { set_err(h, "ft8rx_ft4_ldpc: mask %d outside [0, %d]", mask, FT8RX_MT_ALL); return -1; }
    ENTER(h);
    Scratch S{h};
    float* d_in = S.put(llr, (size_t)n * 174); NEED(d_in);
    float* d_out = S.get<float>((size_t)n * 174); NEED(d_out);
    HIPCHK(h, hipMemset(d_out, 0, sizeof(float) * (size_t)n * 174));
    Att* d_att = S.get<Att>(n); NEED(d_att);
    ft4_launch_bp(h, d_in, n, max_ncheck0, max_iters, (unsigned)mask, d_att, d_out, h->stream);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<Att> a(n);
    HIPCHK(h, hipMemcpy(a.data(), d_att, sizeof(Att) * n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) { ok[i] = a[i].ok; msg_lo[i] = a[i].lo; msg_hi[i] = a[i].hi; n_its[i] = a[i].ok ? a[i].n_its : -1; has_out[i] = a[i].has_out; }
    if (llr_out) HIPCHK(h, hipMemcpy(llr_out, d_out, sizeof(float) * (size_t)n * 174, hipMemcpyDeviceToHost));
    return 0;
}
int ft8rx_ft4_osd(ft8rx_handle* h, const float* llr, int n, int singleflips, int doubleflips, int tripleflips, int max_hd, int32_t mask,
                  int32_t* ok, uint64_t* msg_lo, uint64_t* msg_hi, int32_t* trial, int32_t* hd) {
    if (!h || !llr || n < 1 || !ok || !msg_lo || !msg_hi || !trial) return -1;
    if (mask < 0 || mask > FT8RX_MT_ALL) { set_err(h, "ft8rx_ft4_osd: mask %d outside [0, %d]", mask, FT8RX_MT_ALL); return -1; }
    if (singleflips < 0 || singleflips > OSD_MAXFLIP || doubleflips < 0 || doubleflips > OSD_MAXFLIP || tripleflips < 0 || tripleflips > 40 ||
        max_hd < 0 || max_hd > 174) { set_err(h, "ft8rx_ft4_osd: flip counts out of range"); return -1; }
    const std::vector<uint32_t> tr = osd_trial_table(singleflips, doubleflips, tripleflips);
    if (tr.size() > OSD_MAXTRIALS) { set_err(h, "ft8rx_ft4_osd: %zu trials exceed %d", tr.size(), OSD_MAXTRIALS); return -1; }
    ENTER(h);
    Scratch S{h};
    float* d_in = S.put(llr, (size_t)n * 174); NEED(d_in);
    uint32_t* d_tr = S.put(tr.data(), tr.size()); NEED(d_tr);
    Att* d_att = S.get<Att>(n); NEED(d_att);
    int32_t* d_nan = S.get<int32_t>((size_t)n + 1); NEED(d_nan);
    HIPCHK(h, hipMemsetAsync(d_nan, 0, sizeof(int32_t), h->stream));
    ft4_launch_osd(h, d_in, n, d_tr, (int)tr.size(), osd_nflip(singleflips, tripleflips), max_hd, (unsigned)mask, d_att, d_nan, h->stream);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<Att> a(n);
    HIPCHK(h, hipMemcpy(a.data(), d_att, sizeof(Att) * n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
        ok[i] = a[i].ok; msg_lo[i] = a[i].lo; msg_hi[i] = a[i].hi; trial[i] = a[i].ok ? a[i].n_its : -1;
        if (hd) hd[i] = a[i].ok ? a[i].pad[0] : -1;
    }
    return 0;
}
int ft8rx_ft4_encode_tones(const uint64_t* msg_lo, const uint64_t* msg_hi, int n, uint8_t* tones) {
    if (!msg_lo || !msg_hi || !tones || n < 0) return -1;
    for (int i = 0; i < n; i++) hostmsg::encode_tones_ft4(msg_lo[i], msg_hi[i], tones + (size_t)i * 105);
    return 0;
}

// ---- FT4 subtraction (kernels/ft4_sub.hpp)
#define FT4SUB_MAXSIGS 256
// the BT = 1.0 pulse over three symbols (ft4.py _gfsk_pulse) as its exclusive running sum, [FT4S_PC]
static std::vector<double> ft4_pulse_sums() {
    std::vector<double> pc(FT4S_PC);
    const double k = M_PI * sqrt(2.0 / log(2.0));
    double acc = 0.0;
    for (int i = 0; i < FT4S_PC; i++) {
        pc[i] = acc;
        const double t = ((double)i - 1.5 * FT4_NSPS) / (double)FT4_NSPS;
        acc += 0.5 * (erf(k * (t + 0.5)) - erf(k * (t - 0.5)));
    }
    return pc;
}
// Everything FT4 subtraction owns, at the first ft8rx_ft4_subtract / ft8rx_ft4_sub_probe on the handle, all or nothing
static int ft4sub_workspaces(ft8rx_handle* h) {
    if (ws_ready(h, WS_FT4_SUB)) return 0;
    ft8rx_handle::Ft4Sub& w = h->ft4sub;
    const size_t mf = (size_t)h->max_frames;
    FirstUse F(h, WS_FT4_SUB);
    size_t bytes = 0;
    auto dev = [&](auto** p, size_t n) { F.dev(p, n); bytes += n * sizeof(**p); };
    dev(&w.d_wf, mf * FT8RX_FT4_NSAMP); dev(&w.d_part, mf * FT4S_NT * FT4S_GRIDX * FT4S_NB); dev(&w.d_pc, (size_t)FT4S_PC);
    dev(&w.d_best, mf); dev(&w.d_cnt, mf); dev(&w.d_frame, mf); dev(&w.d_energy, mf * FT4S_NT); dev(&w.d_sigs, mf * FT4SUB_MAXSIGS);
    if (!F.rc) {
        const std::vector<double> pc = ft4_pulse_sums();
        FIRST_HIP(F, hipMemcpy(w.d_pc, pc.data(), sizeof(double) * pc.size(), hipMemcpyHostToDevice));
        FIRST_HIP(F, hipMemset(w.d_best, 0, sizeof(int32_t) * mf));
    }
    const int rc = F.done();
    w.bytes = rc ? 0 : bytes;
    return rc;
}
static Ft4SubShifts ft4sub_shifts(int refine) {
    Ft4SubShifts t;
    t.n = refine ? FT4S_NT : 1;
    for (int i = 0; i < FT4S_NT; i++) t.shift[i] = refine ? 4 * (i - FT4S_NT / 2) : 0;
    return t;
}
// a signal the kernels can walk: tones 0 .. 3, fq x 60480 below 2^31 with room, a start whose sums stay far from overflow
static bool ft4sub_sig_ok(const ft8rx_ft4_subsig& g) {
    if (g.fq < 0 || g.fq >= 4608 || g.start < -(1 << 20) || g.start > (1 << 20)) return false;
    for (int i = 0; i < FT4_NSYM; i++) if (g.tones[i] > 3) return false;
    return true;
}
// signal sel.s of `rows` rows: the trials' bins, the pick (energy: optional [rows][13]), and -- apply -- the subtraction
static void ft4sub_one(ft8rx_handle* h, int rows, const Ft4SubSel& sel, const Ft4SubShifts& sh, double* energy, bool apply) {
    const ft8rx_handle::Ft4Sub& w = h->ft4sub;
    k_ft4_sub_bins<<<dim3(FT4S_GRIDX, rows, sh.n), 256, 0, h->stream>>>(w.d_wf, sel, w.d_pc, sh, w.d_part);
    k_ft4_sub_pick<<<rows, 64, 0, h->stream>>>(sel, sh, w.d_part, w.d_best, energy);
    if (apply) k_ft4_sub_apply<<<dim3(FT4S_GRIDX, rows), 256, 0, h->stream>>>(w.d_wf, sel, w.d_pc, w.d_part, w.d_best);
}

int ft8rx_ft4_subtract(ft8rx_handle* h, int16_t* d_audio, int B, ft8rx_ft4_subsig* sigs, const int32_t* counts, int max_sigs, int refine,
                       float* audio_f32_out) {
    if (!h || !d_audio || !sigs || !counts) return -1;
    if (B < 1 || B > h->max_frames) { set_err(h, "ft8rx_ft4_subtract: n_frames %d outside [1, %d]", B, h->max_frames); return -1; }
    if (max_sigs < 1 || max_sigs > FT4SUB_MAXSIGS) { set_err(h, "ft8rx_ft4_subtract: max_sigs %d outside [1, %d]", max_sigs, FT4SUB_MAXSIGS); return -1; }
    if (refine != 0 && refine != 1) { set_err(h, "ft8rx_ft4_subtract: refine %d is not 0 (the given starts) or 1 (the 13-trial start scan)", refine); return -1; }
    int nmax = 0;
    for (int f = 0; f < B; f++) {
        if (counts[f] < 0 || counts[f] > max_sigs) { set_err(h, "ft8rx_ft4_subtract: counts[%d] = %d outside [0, %d]", f, counts[f], max_sigs); return -1; }
        for (int i = 0; i < counts[f]; i++)
            if (!ft4sub_sig_ok(sigs[(size_t)f * max_sigs + i])) { set_err(h, "ft8rx_ft4_subtract: signal %d of frame %d is out of range (tones 0 .. 3, fq in [0, 4608), |start| <= 2^20)", i, f); return -1; }
        if (counts[f] > nmax) nmax = counts[f];
    }
    ENTER(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (const int rc = ft4sub_workspaces(h)) return rc;
    const ft8rx_handle::Ft4Sub& w = h->ft4sub;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(w.d_sigs, sigs, sizeof(ft8rx_ft4_subsig) * (size_t)B * max_sigs, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(w.d_cnt, counts, sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    const size_t n = (size_t)B * FT8RX_FT4_NSAMP;
    k_sub_to_f32<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_audio, w.d_wf, n);
    const Ft4SubShifts sh = ft4sub_shifts(refine);
    for (int i = 0; i < nmax; i++) ft4sub_one(h, B, Ft4SubSel{w.d_sigs, w.d_cnt, nullptr, max_sigs, i}, sh, nullptr, true);
    k_sub_to_i16<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(w.d_wf, d_audio, n);
    HIPCHK(h, hipGetLastError());
    if (audio_f32_out) HIPCHK(h, hipMemcpyAsync(audio_f32_out, w.d_wf, sizeof(float) * n, hipMemcpyDeviceToHost, s));
    if (refine) HIPCHK(h, hipMemcpyAsync(sigs, w.d_sigs, sizeof(ft8rx_ft4_subsig) * (size_t)B * max_sigs, hipMemcpyDeviceToHost, s));   // the refined starts
    HIPCHK(h, hipStreamSynchronize(s));
    return 0;
}
int ft8rx_ft4_subtraction_list(const ft8rx_record* records, const int32_t* counts, int max_cands, int n_frames, const uint64_t* have_lo,
                               const uint64_t* have_hi, const int32_t* have_counts, int max_have, ft8rx_ft4_subsig* sigs, int max_sigs,
                               int32_t* sig_counts) {
    return hostmsg::ft4_subtraction_list(records, counts, max_cands, n_frames, have_lo, have_hi, have_counts, max_have, sigs, max_sigs, sig_counts);
}
int ft8rx_ft4_sub_info(ft8rx_handle* h, uint64_t* workspace_bytes) {
    if (!h || !workspace_bytes) return -1;
    *workspace_bytes = ws_ready(h, WS_FT4_SUB) ? (uint64_t)h->ft4sub.bytes : 0;
    return 0;
}
int16_t* ft8rx_ft4_staging_audio(ft8rx_handle* h) {
    if (!h || !ws_ready(h, WS_FT4)) return nullptr;
    return h->ft4.d_audio;
}
int ft8rx_ft4_sub_probe(ft8rx_handle* h, const int16_t* audio, int B, int n, const int32_t* frame, const ft8rx_ft4_subsig* sigs, float* model,
                        double* bins, double* energy) {
    if (!ft4_frames_ok(h, "ft8rx_ft4_sub_probe", audio, B) || n < 1 || !frame || !sigs || !bins || !energy) return -1;
    for (int i = 0; i < n; i++)
        if (frame[i] < 0 || frame[i] >= B || !ft4sub_sig_ok(sigs[i])) {
            set_err(h, "ft8rx_ft4_sub_probe: signal %d (frame %d) is out of range (tones 0 .. 3, fq in [0, 4608), |start| <= 2^20)", i, frame[i]); return -1; }
    ENTER(h);
    if (const int rc = ft4_workspaces(h)) return rc;
    if (const int rc = ft4sub_workspaces(h)) return rc;
    const ft8rx_handle::Ft4Sub& w = h->ft4sub;
    hipStream_t s = h->stream;
    const size_t na = (size_t)B * FT8RX_FT4_NSAMP;
    HIPCHK(h, hipMemcpy(h->ft4.d_audio, audio, sizeof(int16_t) * na, hipMemcpyHostToDevice));
    k_sub_to_f32<<<(unsigned)((na + 255) / 256), 256, 0, s>>>(h->ft4.d_audio, w.d_wf, na);
    Scratch S{h};
    float2* d_model = nullptr;
    if (model) { d_model = S.get<float2>((size_t)h->max_frames * FT4S_N); NEED(d_model); }
    const std::vector<int32_t> ones((size_t)h->max_frames, 1);
    HIPCHK(h, hipMemcpyAsync(w.d_cnt, ones.data(), sizeof(int32_t) * ones.size(), hipMemcpyHostToDevice, s));
    const Ft4SubShifts sh = ft4sub_shifts(1);
    std::vector<double2> part((size_t)FT4S_NT * FT4S_GRIDX * FT4S_NB);
    for (int i0 = 0; i0 < n; i0 += h->max_frames) {                       // the signals in slabs of max_frames rows, one signal per row
        const int rows = n - i0 < h->max_frames ? n - i0 : h->max_frames;
        HIPCHK(h, hipMemcpyAsync(w.d_sigs, sigs + i0, sizeof(ft8rx_ft4_subsig) * rows, hipMemcpyHostToDevice, s));
        HIPCHK(h, hipMemcpyAsync(w.d_frame, frame + i0, sizeof(int32_t) * rows, hipMemcpyHostToDevice, s));
        const Ft4SubSel sel{w.d_sigs, w.d_cnt, w.d_frame, 1, 0};
        if (model) k_ft4_sub_model<<<dim3(FT4S_GRIDX, rows), 256, 0, s>>>(sel, w.d_pc, d_model);
        ft4sub_one(h, rows, sel, sh, w.d_energy, false);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamSynchronize(s));
        if (model) HIPCHK(h, hipMemcpy(model + (size_t)i0 * FT4S_N * 2, d_model, sizeof(float2) * (size_t)rows * FT4S_N, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(energy + (size_t)i0 * FT4S_NT, w.d_energy, sizeof(double) * (size_t)rows * FT4S_NT, hipMemcpyDeviceToHost));
        for (int r = 0; r < rows; r++) {                                  // the bins at the given start: trial 6 (shift 0), the partials in block order
            HIPCHK(h, hipMemcpy(part.data(), w.d_part + (size_t)r * part.size(), sizeof(double2) * part.size(), hipMemcpyDeviceToHost));
            for (int b = 0; b < FT4S_NB; b++) {
                double vr = 0.0, vi = 0.0;
                for (int c = 0; c < FT4S_GRIDX; c++) { const double2 v = part[((size_t)(FT4S_NT / 2) * FT4S_GRIDX + c) * FT4S_NB + b]; vr += v.x; vi += v.y; }
                bins[((size_t)(i0 + r) * FT4S_NB + b) * 2] = vr; bins[((size_t)(i0 + r) * FT4S_NB + b) * 2 + 1] = vi;
            }
        }
    }
    return 0;
}

// ---- FT4 measured reports (kernels/ft4_report.hpp)
#define FT4REP_ROWS 32               /* rows of a slab per frame of max_frames */
// Everything the FT4 reports own, at the first ft8rx_ft4_report on the handle, all or nothing
static int ft4rep_workspaces(ft8rx_handle* h) {
    if (ws_ready(h, WS_FT4_REPORT)) return 0;
    ft8rx_handle::Ft4Rep& w = h->ft4rep;
    const size_t mf = (size_t)h->max_frames, nr = mf * FT4REP_ROWS;
    FirstUse F(h, WS_FT4_REPORT);
    size_t bytes = 0;
    auto dev = [&](auto** p, size_t n) { F.dev(p, n); bytes += n * sizeof(**p); };
    dev(&w.d_wf, mf * FT8RX_FT4_NSAMP); dev(&w.d_pc, (size_t)FT4S_PC); dev(&w.d_sigs, nr); dev(&w.d_frame, nr); dev(&w.d_one, nr);
    dev(&w.d_part, nr * FT4R_NBLK * FT4R_NP); dev(&w.d_scores, nr * FT4R_NP); dev(&w.d_peak, nr); dev(&w.d_rep, nr); dev(&w.d_onoff, nr * 2);
    if (!F.rc) {
        const std::vector<double> pc = ft4_pulse_sums();
        const std::vector<int32_t> ones(nr, 1);
        FIRST_HIP(F, hipMemcpy(w.d_pc, pc.data(), sizeof(double) * pc.size(), hipMemcpyHostToDevice));
        FIRST_HIP(F, hipMemcpy(w.d_one, ones.data(), sizeof(int32_t) * nr, hipMemcpyHostToDevice));
    }
    const int rc = F.done();
    w.bytes = rc ? 0 : bytes;
    return rc;
}
int ft8rx_ft4_report(ft8rx_handle* h, const int16_t* d_audio, int B, const ft8rx_ft4_subsig* sigs, const int32_t* counts, int max_sigs, int n_have,
                     ft8rx_report* reports, float* scores, float* on_off) {
    if (!h || !d_audio || !sigs || !counts || !reports) return -1;
    if (B < 1 || B > h->max_frames) { set_err(h, "ft8rx_ft4_report: n_frames %d outside [1, %d]", B, h->max_frames); return -1; }
    if (max_sigs < 1) { set_err(h, "ft8rx_ft4_report: max_sigs %d is below 1", max_sigs); return -1; }
    if (n_have < FT4_NSPS || n_have > FT8RX_FT4_NSAMP) { set_err(h, "ft8rx_ft4_report: n_have %d outside [%d, %d]", n_have, FT4_NSPS, FT8RX_FT4_NSAMP); return -1; }
    std::vector<int32_t> frame, slot;                                     // the live signals, one per row, in (frame, signal) order
    for (int f = 0; f < B; f++) {
        if (counts[f] < 0 || counts[f] > max_sigs) { set_err(h, "ft8rx_ft4_report: counts[%d] = %d outside [0, %d]", f, counts[f], max_sigs); return -1; }
        for (int i = 0; i < counts[f]; i++) {
            const ft8rx_ft4_subsig& g = sigs[(size_t)f * max_sigs + i];
            for (int k = 0; k < FT4_NSYM; k++)
                if (g.tones[k] > 3) { set_err(h, "ft8rx_ft4_report: signal %d of frame %d: tone %d of symbol %d is above 3", i, f, (int)g.tones[k], k); return -1; }
            if (g.fq < 0 || g.fq >= 4608) { set_err(h, "ft8rx_ft4_report: signal %d of frame %d: fq %d outside [0, 4608)", i, f, g.fq); return -1; }
            if (g.start < -(1 << 20) || g.start > (1 << 20)) { set_err(h, "ft8rx_ft4_report: signal %d of frame %d: |start| %d above 2^20", i, f, g.start); return -1; }
            frame.push_back(f); slot.push_back(f * max_sigs + i);
        }
    }
    ENTER(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (const int rc = ft4rep_workspaces(h)) return rc;
    const ft8rx_handle::Ft4Rep& w = h->ft4rep;
    hipStream_t s = h->stream;
    const size_t total = (size_t)B * max_sigs;
    memset(reports, 0, sizeof(ft8rx_report) * total);
    if (scores) memset(scores, 0, sizeof(float) * total * FT4R_NP);
    if (on_off) memset(on_off, 0, sizeof(float) * total * 2);
    // profiling (ft8rx_set_profiling): the stages of the first slab, read like a batch's after ft8rx_sync
    h->pnames.clear();
    const bool prof = h->profiling;
    bool first = true;
#define STAGE(name) do { if (prof && first) { hipEventRecord(h->pev[h->pnames.size()], s); h->pnames.push_back(name); } } while (0)
    STAGE("ft4_rep_f32");
    k_ft4_rep_f32<<<dim3((FT8RX_FT4_NSAMP + 255) / 256, B), 256, 0, s>>>(d_audio, w.d_wf, n_have);
    const size_t cap = (size_t)h->max_frames * FT4REP_ROWS, n = frame.size();
    std::vector<ft8rx_ft4_subsig> slab(cap);
    std::vector<ft8rx_report> rp(cap);
    std::vector<float> sc(scores ? cap * FT4R_NP : 0), oo(on_off ? cap * 2 : 0);
    const Ft4SubSel sel{w.d_sigs, w.d_one, w.d_frame, 1, 0};
    for (size_t i0 = 0; i0 < n; i0 += cap) {
        const int rows = (int)(n - i0 < cap ? n - i0 : cap);
        for (int r = 0; r < rows; r++) slab[r] = sigs[slot[i0 + r]];
        HIPCHK(h, hipMemcpyAsync(w.d_sigs, slab.data(), sizeof(ft8rx_ft4_subsig) * rows, hipMemcpyHostToDevice, s));
        HIPCHK(h, hipMemcpyAsync(w.d_frame, frame.data() + i0, sizeof(int32_t) * rows, hipMemcpyHostToDevice, s));
        STAGE("ft4_rep_scan");
        k_ft4_rep_scan<<<dim3(FT4R_NBLK / 2, rows), 128, 0, s>>>(w.d_wf, sel, w.d_pc, w.d_part);
        STAGE("ft4_rep_pick");
        k_ft4_rep_pick<<<rows, 64, 0, s>>>(sel, w.d_part, w.d_scores, w.d_peak);
        STAGE("ft4_rep_snr");
        k_ft4_rep_snr<<<rows, 256, 0, s>>>(w.d_wf, sel, w.d_pc, w.d_peak, n_have, w.d_rep, w.d_onoff);
        if (prof && first) hipEventRecord(h->pev[h->pnames.size()], s);
        first = false;
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(rp.data(), w.d_rep, sizeof(ft8rx_report) * rows, hipMemcpyDeviceToHost, s));
        if (scores) HIPCHK(h, hipMemcpyAsync(sc.data(), w.d_scores, sizeof(float) * (size_t)rows * FT4R_NP, hipMemcpyDeviceToHost, s));
        if (on_off) HIPCHK(h, hipMemcpyAsync(oo.data(), w.d_onoff, sizeof(float) * (size_t)rows * 2, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        for (int r = 0; r < rows; r++) {
            const size_t o = (size_t)slot[i0 + r];
            reports[o] = rp[r];
            if (scores) memcpy(scores + o * FT4R_NP, sc.data() + (size_t)r * FT4R_NP, sizeof(float) * FT4R_NP);
            if (on_off) { on_off[2 * o] = oo[2 * (size_t)r]; on_off[2 * o + 1] = oo[2 * (size_t)r + 1]; }
        }
    }
    if (prof && first) hipEventRecord(h->pev[h->pnames.size()], s);      // no signal at all: the conversion is the only stage
#undef STAGE
    HIPCHK(h, hipStreamSynchronize(s));
    return 0;
}
int ft8rx_ft4_report_info(ft8rx_handle* h, uint64_t* workspace_bytes) {
    if (!h || !workspace_bytes) return -1;
    *workspace_bytes = ws_ready(h, WS_FT4_REPORT) ? (uint64_t)h->ft4rep.bytes : 0;
    return 0;
}

int16_t* ft8rx_staging_audio(ft8rx_handle* h) {
    if (!h || hipSetDevice(h->device) != hipSuccess || need_staging(h)) return nullptr;
    return h->d_audio;
}
float* ft8rx_staging_audio_f32(ft8rx_handle* h) {
    if (!h || hipSetDevice(h->device) != hipSuccess || need_staging_f32(h)) return nullptr;
    return h->d_audio_f;
}

// Asynchronous D2H copies for a consumer of device-side results (the gather on rank `dst`, pyft8_amd/distributed.py), on the handle's
// RESULT-COPY stream: the one stream of the handle no decode kernel ever waits behind.  The runtime maps streams onto four hardware
// queues and the commands of a queue execute in order, so a copy issued on any OTHER stream of the process (a torch side stream)
// lands in a queue it shares with one of the decode streams and holds that stream's kernels back for as long as it runs -- 12 MB per
// step (rank 0's load in an 8-GPU config-1 job) cost 4.7 % of the step that way (profiles/r06_notes.md).
int ft8rx_d2h_async(ft8rx_handle* h, void* dst, const void* d_src, uint64_t bytes, int32_t* ticket) {
    if (!h || !dst || !d_src || !ticket) return -1;
    HIPCHK(h, hipSetDevice(h->device));
    const uint32_t id = h->d2h_next;
    hipEvent_t& e = h->d2h_ev[id & 31];
    if (!e) HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    else if (id >= 32 && hipEventQuery(e) == hipErrorNotReady) HIPCHK(h, hipEventSynchronize(e));      // 32 copies in flight: wait for the oldest
    if (bytes) HIPCHK(h, hipMemcpyAsync(dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost, h->copy_s));
    HIPCHK(h, hipEventRecord(e, h->copy_s));
    h->d2h_next = id + 1;
    *ticket = (int32_t)(id & 0x7fffffffu);
    return 0;
}
int ft8rx_d2h_query(ft8rx_handle* h, int32_t ticket) {              // 1 = the copy has landed, 0 = not yet, < 0 = error
    if (!h || ticket < 0) return -1;
    const uint32_t id = (uint32_t)ticket, next = h->d2h_next & 0x7fffffffu;
    const uint32_t age = (next - id) & 0x7fffffffu;
    if (age == 0u || age > 0x40000000u) { set_err(h, "ft8rx_d2h_query: ticket %d was never issued", ticket); return -1; }
    if (age > 32u) return 1;                                        // its event has been reused since: long done
    const hipError_t r = hipEventQuery(h->d2h_ev[id & 31]);
    if (r == hipSuccess) return 1;
    if (r == hipErrorNotReady) return 0;
    set_err(h, "ft8rx_d2h_query: %s", hipGetErrorString(r));
    return -2;
}
void* ft8rx_d2h_event(ft8rx_handle* h, int32_t ticket) {            // the HIP event behind that copy (for ft8rx_packed_output_fence), or NULL
    if (!h || ticket < 0) return nullptr;
    const uint32_t id = (uint32_t)ticket, next = h->d2h_next & 0x7fffffffu;
    const uint32_t age = (next - id) & 0x7fffffffu;
    return (age >= 1u && age <= 32u) ? (void*)h->d2h_ev[id & 31] : nullptr;
}

int ft8rx_copy_to_host(ft8rx_handle* h, void* dst, const void* d_src, uint64_t bytes) {
    if (!h || !dst || !d_src) return -1;
    ENTER(h);
    HIPCHK(h, hipMemcpy(dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost));
    return 0;
}

// ft8rx_subtract's workspaces, each group on first use: the float32 working copy, partial sums and GFSK pulse tables
// (transmitter.py:41-50) for max_frames frames; refine = 2: the decimated baseband copy; refine = 3: an all-ones taper table
static int subtract_workspaces(ft8rx_handle* h, int refine) {
    const size_t MB = (size_t)h->max_frames;
    if (!ws_ready(h, WS_SUB)) {
        FirstUse F(h, WS_SUB);
        F.dev(&h->d_wf, MB * FT8RX_NSAMP);
        F.dev(&h->d_part, MB * SUB_NCH * 20);           // also holds the refinement scan: [SUB_MAXSHIFT][SUB_NCH] <= [SUB_NCH][20]
        F.dev(&h->d_pulse, (size_t)5760);
        F.dev(&h->d_pc, (size_t)5760);
        F.dev(&h->d_sigcnt, MB);
        std::vector<double> pulse(5760), pc(5760);
        const double c = M_PI * sqrt(2.0 / log(2.0)), bt = 2.0;
        double acc = 0.0;
        for (int i = 0; i < 5760; i++) {
            const double tt = ((double)i - 1.5 * 1920.0) / 1920.0;
            pulse[i] = 0.5 * (erf(c * bt * (tt + 0.5)) - erf(c * bt * (tt - 0.5)));
            acc += pulse[i]; pc[i] = acc;
        }
        FIRST_HIP(F, hipMemcpy(h->d_pulse, pulse.data(), sizeof(double) * 5760, hipMemcpyHostToDevice));
        FIRST_HIP(F, hipMemcpy(h->d_pc, pc.data(), sizeof(double) * 5760, hipMemcpyHostToDevice));
        if (F.done()) return -2;
    }
    if (refine == 2 && !ws_ready(h, WS_SUBD)) {
        FirstUse F(h, WS_SUBD);
        F.dev(&h->d_zdec, MB * SUBD_NZ);
        F.dev(&h->d_model, MB * SUBD_N);
        F.dev(&h->d_adec, MB * (SUBD_N + 1));
        F.dev(&h->d_subctx, MB);
        if (F.done()) return -2;
    }
    if (refine == 3 && !ws_ready(h, WS_ONES)) {
        FirstUse F(h, WS_ONES);
        F.dev(&h->d_ones, (size_t)100);
        double ones[100]; for (int i = 0; i < 100; i++) ones[i] = 1.0;
        FIRST_HIP(F, hipMemcpy(h->d_ones, ones, sizeof(ones), hipMemcpyHostToDevice));
        if (F.done()) return -2;
    }
    return 0;
}

// The refinement scans of ft8rx_subtract: coarse (10 ms / 0.25 Hz around the decoder's origin, which by the search-grid conventions
// sits ~75 ms late and ~1.9 Hz low), then fine (2.5 ms / 0.0625 Hz); decimated = refine 2's, the same steps on a decimated baseband
// copy (kernels/subtract.hpp): time shifts in units of 32 samples
// (decimating the scan itself, every 8th / 2nd sample, was tried: it aliases neighbouring signals into the sums, 1 of 233 origins locked 70 ms off)
static SubShifts sub_shifts(bool decimated, bool fine) {
    SubShifts t;
    for (int i = 0; i < SUB_MAXSHIFT; i++) t.shift[i] = 0;
    if (fine) { t.n = 9; for (int i = 0; i < 9; i++) t.shift[i] = decimated ? SUBD_D * (-4 + i) : -120 + 30 * i; }       // -10 .. +10 ms (decimated: -10.7 .. +10.7 ms in 2.67 ms steps)
    else if (decimated) { t.n = 15; for (int i = 0; i < 15; i++) t.shift[i] = SUBD_D * (-52 + 4 * i); }                   // -138.7 .. +10.7 ms in 10.7 ms steps
    else { t.n = 16; for (int i = 0; i < 16; i++) t.shift[i] = -1680 + 120 * i; }                                        // -140 .. +10 ms
    return t;
}
// ... and the frequency grid k_sub_pick tries with each: df = df_lo + df_step * [0, ndf)
static const struct { float df_lo, df_step; int ndf; } SUB_GRID[2] = {
    {-1.0f, 0.0625f, 113},         // coarse: signal - model = -1 .. +6 Hz; the sum is coherent over 12.6 s, so the grid must be as fine as 1/16 Hz
    {0.4375f, 0.015625f, 9},       // fine: around the +0.5 Hz the coarse step left
};
static_assert(SUB_MAXSHIFT * SUB_NCH <= SUB_NCH * 20, "the refinement scan [SUB_MAXSHIFT][SUB_NCH] lives in d_part [SUB_NCH][20]");

// refine 1 / 2: coarse scan, pick, fine scan, pick for signal sel.s of B frames; decimated = on the baseband copy k_subd_mix made
static void sub_refine(ft8rx_handle* h, int B, const SubSel& sel, const SubTables& T, bool decimated) {
    for (int fine = 0; fine < 2; fine++) {
        const SubShifts sh = sub_shifts(decimated, fine);
        if (decimated) {
            k_subd_model<<<dim3((SUBD_N + 255) / 256, B), 256, 0, h->stream>>>(sel, T, h->d_subctx, h->d_model);
            k_subd_scan<<<B, 256, 0, h->stream>>>(h->d_zdec, h->d_model, sel, h->d_subctx, sh, h->d_part);
        } else k_sub_scan<<<dim3(SUB_GRIDX, B), 256, 0, h->stream>>>(h->d_wf, sel, T, sh, h->d_part);
        k_sub_pick<<<B, 256, 0, h->stream>>>(sel, sh, h->d_part, SUB_GRID[fine].df_lo, SUB_GRID[fine].df_step, SUB_GRID[fine].ndf,
                                             decimated ? SUBD_D * SUBD_CH : SUB_CH);
    }
}
// the reference's subtract_signal at full rate
static void sub_apply_fullrate(ft8rx_handle* h, int B, const SubSel& sel, const SubTables& T) {
    k_sub_accum<<<dim3(SUB_GRIDX, B), 256, 0, h->stream>>>(h->d_wf, sel, T, h->d_part);
    k_sub_apply<<<dim3(SUB_GRIDX, B), 256, 0, h->stream>>>(h->d_wf, sel, T, h->d_part);
}

// the two entries: int16 frames (converted into the float32 working copy and rounded back), or float32 frames (d_f32: copied into the
// working copy and back as they are); everything between those two steps is the same
static int subtract_run(ft8rx_handle* h, const char* who, int16_t* d_audio, float* d_f32, int B, ft8rx_subsig* sigs, const int32_t* counts,
                        int max_sigs, int refine, float* audio_f32_out) {
    if (!h || (!d_audio && !d_f32) || !sigs || !counts) return -1;
    if (B < 1 || B > h->max_frames || max_sigs < 1 || max_sigs > 256 || refine < 0 || refine > 3) { set_err(h, "%s: bad n_frames / max_sigs / refine", who); return -1; }
    ENTER(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (subtract_workspaces(h, 0)) return -2;           // the base group; the groups of refine 2 / 3 follow the audio's conversion, below
    if (h->sig_cap < max_sigs) {
        ft8rx_subsig* p = nullptr;
        if (dalloc(h, &p, (size_t)h->max_frames * max_sigs)) return -2;       // the smaller one stays in the handle's allocation list
        h->d_sigs = p; h->sig_cap = max_sigs;
    }
    int nmax = 0;
    for (int f = 0; f < B; f++) {
        if (counts[f] < 0 || counts[f] > max_sigs) { set_err(h, "%s: counts[%d] = %d outside [0, %d]", who, f, counts[f], max_sigs); return -1; }
        if (counts[f] > nmax) nmax = counts[f];
    }
    HIPCHK(h, hipMemcpyAsync(h->d_sigs, sigs, sizeof(ft8rx_subsig) * (size_t)B * max_sigs, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_sigcnt, counts, sizeof(int32_t) * B, hipMemcpyHostToDevice, h->stream));
    const size_t n = (size_t)B * FT8RX_NSAMP;
    if (d_f32) HIPCHK(h, hipMemcpyAsync(h->d_wf, d_f32, sizeof(float) * n, hipMemcpyDeviceToDevice, h->stream));
    else k_sub_to_f32<<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(d_audio, h->d_wf, n);
    if (subtract_workspaces(h, refine)) return -2;
    const SubTables T{h->d_pulse, h->d_pc};
    Tables Tones = h->T;                                     // refine = 3: the experiment's slices have no edge tapers
    if (refine == 3) Tones.taper = h->d_ones;
    for (int s = 0; s < nmax; s++) {
        const SubSel sel{h->d_sigs, h->d_sigcnt, max_sigs, s};
        if (refine == 2) {                                   // everything but the subtraction itself on the decimated baseband copy
            k_subd_mix<<<dim3(SUBD_NZ / 256, B), 256, 0, h->stream>>>(h->d_wf, sel, h->d_zdec, h->d_subctx);
            sub_refine(h, B, sel, T, true);
            k_subd_model<<<dim3((SUBD_N + 255) / 256, B), 256, 0, h->stream>>>(sel, T, h->d_subctx, h->d_model);
            k_subd_accum<<<B, 256, 0, h->stream>>>(h->d_zdec, h->d_model, sel, h->d_subctx, h->d_adec);
            k_subd_apply<<<dim3(SUB_GRIDX, B), 256, 0, h->stream>>>(h->d_wf, sel, T, h->d_adec);
            continue;
        }
        if (refine == 1) sub_refine(h, B, sel, T, false);
        if (refine == 3) {
            // Candidate.refine_time_origin (receiver_sub.py:58-72) on the spectrum of the residual so far, then subtract_signal as is
            k_cyc_a_f32<<<dim3(40, B), 256, 0, h->stream>>>(h->d_wf, h->d_A, h->T);
            k_cyc_bc<<<dim3(CYC_BC_GRID, B), 256, 0, h->stream>>>(h->d_A, h->d_spec, h->T);
            k_refine3<<<B, FINE_NT, 0, h->stream>>>(h->d_spec, sel, Tones);
        }
        sub_apply_fullrate(h, B, sel, T);
    }
    if (d_f32) HIPCHK(h, hipMemcpyAsync(d_f32, h->d_wf, sizeof(float) * n, hipMemcpyDeviceToDevice, h->stream));
    else k_sub_to_i16<<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(h->d_wf, d_audio, n);
    HIPCHK(h, hipGetLastError());
    if (audio_f32_out) HIPCHK(h, hipMemcpyAsync(audio_f32_out, h->d_wf, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    if (refine) HIPCHK(h, hipMemcpyAsync(sigs, h->d_sigs, sizeof(ft8rx_subsig) * (size_t)B * max_sigs, hipMemcpyDeviceToHost, h->stream));   // the refined origins
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}
int ft8rx_subtract(ft8rx_handle* h, int16_t* d_audio, int B, ft8rx_subsig* sigs, const int32_t* counts, int max_sigs,
                   int refine, float* audio_f32_out) {
    if (!d_audio) return -1;
    return subtract_run(h, "ft8rx_subtract", d_audio, nullptr, B, sigs, counts, max_sigs, refine, audio_f32_out);
}
int ft8rx_subtract_f32(ft8rx_handle* h, float* d_audio, int B, ft8rx_subsig* sigs, const int32_t* counts, int max_sigs,
                       int refine, float* audio_f32_out) {
    if (!d_audio) return -1;
    if (h && ((uintptr_t)d_audio % sizeof(float)) != 0) { set_err(h, "ft8rx_subtract_f32: d_audio is not aligned to a sample"); return -1; }
    return subtract_run(h, "ft8rx_subtract_f32", nullptr, d_audio, B, sigs, counts, max_sigs, refine, audio_f32_out);
}

int ft8rx_encode_tones(const uint64_t* msg_lo, const uint64_t* msg_hi, int n, uint8_t* tones) {
    if (!msg_lo || !msg_hi || !tones || n < 0) return -1;
    for (int i = 0; i < n; i++) hostmsg::encode_tones(msg_lo[i], msg_hi[i], tones + (size_t)i * 79);
    return 0;
}

void* ft8rx_alloc_host(ft8rx_handle* h, uint64_t bytes) {
    if (!h || bytes == 0) return nullptr;
    void* p = nullptr;
    if (hipSetDevice(h->device) != hipSuccess || hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) != hipSuccess) {
        set_err(h, "ft8rx_alloc_host: hipHostMalloc(%llu) failed", (unsigned long long)bytes);
        return nullptr;
    }
    return p;
}

int ft8rx_free_host(ft8rx_handle* h, void* p) {          // h may be NULL (buffers can outlive the handle that allocated them)
    if (!p) return -1;
    const hipError_t e = hipHostFree(p);
    if (e != hipSuccess) { if (h) set_err(h, "hipHostFree failed: %s", hipGetErrorString(e)); return -2; }
    return 0;
}

int ft8rx_synth_frames_ex(ft8rx_handle* h, uint64_t seed, int first_index, int n_frames, int n_signals,
                          const void* signal_table, int signal_bytes, const double* pulse_cumsum, int16_t* d_audio, int no_noise) {
    if (!h || !signal_table || !pulse_cumsum || !d_audio || n_frames < 1 || n_signals < 0 || n_signals > 64) return -1;
    if (signal_bytes != (int)sizeof(SynthSig)) { set_err(h, "ft8rx_synth_frames: signal record is %d bytes, expected %d", signal_bytes, (int)sizeof(SynthSig)); return -1; }
    ENTER(h);
    Scratch S{h};
    SynthSig* d_s = S.put((const SynthSig*)signal_table, (size_t)n_frames * (n_signals ? n_signals : 1)); NEED(d_s);
    double* d_q = S.put(pulse_cumsum, 5761); NEED(d_q);
    k_synth<<<dim3((FT8RX_NSAMP / 4 + 255) / 256, n_frames), 256, 0, h->stream>>>(d_audio, d_s, n_signals, d_q, (uint32_t)seed, (uint32_t)(seed >> 32), first_index, no_noise);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int ft8rx_synth_frames(ft8rx_handle* h, uint64_t seed, int first_index, int n_frames, int n_signals,
                       const void* signal_table, int signal_bytes, const double* pulse_cumsum, int16_t* d_audio) {
    return ft8rx_synth_frames_ex(h, seed, first_index, n_frames, n_signals, signal_table, signal_bytes, pulse_cumsum, d_audio, 0);
}

int ft8rx_package_batch(const ft8rx_record* records, const int32_t* counts, const ft8rx_event* events, const int32_t* event_counts,
                        int n_frames, int max_cands, ft8rx_message* out, int max_msgs, int32_t* out_counts, int n_threads,
                        ft8rx_hashes* table, int32_t* flags) {
    return hostmsg::package_batch(records, counts, events, event_counts, n_frames, max_cands, out, max_msgs, out_counts, n_threads,
                                  table ? &table->H : nullptr, flags);
}

int ft8rx_package_batch_ext(const ft8rx_record* records, const int32_t* counts, const ft8rx_event* events, const int32_t* event_counts,
                            int n_frames, int max_cands, ft8rx_message_ext* out, int max_msgs, int32_t* out_counts, int n_threads,
                            ft8rx_hashes* table, int32_t* flags, int32_t mask) {
    if (mask < 0 || mask > FT8RX_MT_ALL) return -1;
    return hostmsg::package_batch(records, counts, events, event_counts, n_frames, max_cands, out, max_msgs, out_counts, n_threads,
                                  table ? &table->H : nullptr, flags, (unsigned)mask);
}

int ft8rx_package_batch_recall(const ft8rx_record* records, const int32_t* counts, const ft8rx_event* events, const int32_t* event_counts,
                               const ft8rx_record* recall, const int32_t* recall_counts, int n_frames, int max_cands, ft8rx_message* out,
                               int max_msgs, int32_t* out_counts, int n_threads, ft8rx_hashes* table, int32_t* flags) {
    if (!recall || !recall_counts) return -1;
    return hostmsg::package_batch(records, counts, events, event_counts, n_frames, max_cands, out, max_msgs, out_counts, n_threads,
                                  table ? &table->H : nullptr, flags, 0u, recall, recall_counts);
}

int ft8rx_package_packed(const void* packed, uint64_t bytes, int frame_lo, int n_frames, ft8rx_message* out, int max_msgs,
                         int32_t* out_counts, int n_threads, ft8rx_hashes* table, int32_t* flags) {
    return hostmsg::package_packed(packed, bytes, frame_lo, n_frames, out, max_msgs, out_counts, n_threads, table ? &table->H : nullptr, flags);
}

int ft8rx_merge_messages(ft8rx_message* out, int32_t* out_counts, int max_out, const ft8rx_message* add, const int32_t* add_counts,
                         int max_add, int n_frames, int pass_tag, int drop_osd, ft8rx_message* fresh, int32_t* fresh_counts) {
    if (!out || !out_counts || !add || !add_counts || n_frames < 0 || max_out < 1 || max_add < 1) return -1;
    hostmsg::merge_messages(out, out_counts, max_out, add, add_counts, max_add, n_frames, pass_tag, drop_osd, fresh, fresh_counts);
    return 0;
}

int ft8rx_subtraction_list(const ft8rx_message* msgs, const int32_t* counts, int max_msgs, const ft8rx_record* records, int max_cands,
                           int n_frames, int min_snr, ft8rx_subsig* sigs, int max_sigs, int32_t* sig_counts) {
    if (!msgs || !counts || !records || !sigs || !sig_counts || n_frames < 0 || max_msgs < 1 || max_cands < 1 || max_sigs < 1) return -1;
    return hostmsg::subtraction_list(msgs, counts, max_msgs, records, max_cands, n_frames, min_snr, sigs, max_sigs, sig_counts);
}

ft8rx_hashes* ft8rx_hashes_create(void) { return new (std::nothrow) ft8rx_hashes(); }
void ft8rx_hashes_destroy(ft8rx_hashes* t) { delete t; }
int ft8rx_hashes_clear(ft8rx_hashes* t) { if (!t) return -1; t->H.clear(); return 0; }
int ft8rx_hashes_add(ft8rx_hashes* t, const char* call) { if (!t || !call) return -1; t->H.add(call); return 0; }
int ft8rx_hashes_size(const ft8rx_hashes* t) { return t ? (int)t->H.size() : -1; }

int ft8rx_set_reject_log(const char* path) { hostmsg::set_reject_log(path); return 0; }

#ifdef FINE_TIMING
int ft8rx_debug_fine_times(ft8rx_handle* h, unsigned long long* out32, int reset) {      // timing-only builds (tools/fine_timing.sh)
    if (!h) return -1;
    ENTER(h);
    return ft8rx_ilp_fine_times(out32, reset);          // the instrumented kernel lives in the second translation unit
}
#endif

#ifdef BP_TIMING
int ft8rx_debug_bp_times(ft8rx_handle* h, unsigned long long* out8, int reset) {         // timing-only builds (tools/bp_timing.py)
    if (!h) return -1;
    ENTER(h);
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    std::vector<unsigned long long> all((size_t)65536 * 8);
    if (out8) {
        if (hipMemcpyFromSymbol(all.data(), HIP_SYMBOL(g_bp_t), sizeof(unsigned long long) * all.size()) != hipSuccess) return -2;
        for (int i = 0; i < 8; i++) out8[i] = 0;
        for (size_t b = 0; b < 65536; b++) for (int i = 0; i < 8; i++) out8[i] += all[b * 8 + i];
    }
    if (reset) { std::fill(all.begin(), all.end(), 0ull); if (hipMemcpyToSymbol(HIP_SYMBOL(g_bp_t), all.data(), sizeof(unsigned long long) * all.size()) != hipSuccess) return -2; }
    return 0;
}
#endif
#ifdef OSD_TIMING
int ft8rx_debug_osd_times(ft8rx_handle* h, unsigned long long* out16, int reset) {       // timing-only builds (tools/osd_timing.py)
    if (!h) return -1;
    ENTER(h);
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    std::vector<unsigned long long> all((size_t)32768 * 10);
    if (out16) {
        if (hipMemcpyFromSymbol(all.data(), HIP_SYMBOL(g_osd_t), sizeof(unsigned long long) * all.size()) != hipSuccess) return -2;
        for (int i = 0; i < 16; i++) out16[i] = 0;
        for (size_t b = 0; b < 32768; b++) for (int i = 0; i < 10; i++) out16[i == 9 ? 15 : i] += all[b * 10 + i];
    }
    if (reset) { std::fill(all.begin(), all.end(), 0ull); if (hipMemcpyToSymbol(HIP_SYMBOL(g_osd_t), all.data(), sizeof(unsigned long long) * all.size()) != hipSuccess) return -2; }
    return 0;
}
#endif

int ft8rx_math_probe(ft8rx_handle* h, int which, const float* x, int n, float* y) {
    if (!h || !x || !y || n < 1) return -1;
    ENTER(h);
    Scratch S{h};
    if (which == 0 || which == 1) {
        float* d_x = S.put(x, n); NEED(d_x);
        float* d_y = S.get<float>(n); NEED(d_y);
        k_math_probe<<<(n + 255) / 256, 256, 0, h->stream>>>(which, d_x, d_y, n);
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(y, d_y, sizeof(float) * n, hipMemcpyDeviceToHost));
        return 0;
    }
    if (which == 2) {
        cpx* d_x = S.put((const cpx*)x, n); NEED(d_x);
        cpx* d_y = S.get<cpx>(n); NEED(d_y);
        const size_t lds = 2 * (size_t)n * sizeof(cpx);
        if (n == 1920) k_fft_probe<1920, 8, 4, 4, 5, 3><<<1, 256, lds, h->stream>>>(d_x, d_y, h->T.W1920);
        else if (n == 3200) k_fft_probe<3200, 8, 4, 4, 5, 5><<<1, 256, lds, h->stream>>>(d_x, d_y, h->T.W3200);
        else if (n == 300) k_fft_probe<300, 5, 5, 4, 3><<<1, 256, lds, h->stream>>>(d_x, d_y, h->T.W300);
        else if (n == 320) k_fft_probe<320, 8, 8, 5><<<1, 256, lds, h->stream>>>(d_x, d_y, h->T.W320);
        else { set_err(h, "ft8rx_math_probe: no FFT plan of length %d", n); return -1; }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(y, d_y, sizeof(cpx) * n, hipMemcpyDeviceToHost));
        return 0;
    }
    return -1;
}

}  // extern "C"
