/* ft8rx.h -- C ABI of libft8rx.so: the MI355X-native FT8 receive hot path.
 *
 * The reference (G1OJS/PyFT8) is pure Python and has no FFI for this path; its boundary is the
 * Python surface of PyFT8/receiver.py + PyFT8/decoders.py.  Each entry point
 * below names the reference interface it stands in for; pyft8_amd/{receiver,decoders}.py bind
 * them with ctypes and re-create that Python surface.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function returns 0 on
 * success and a negative code on failure (ft8rx_last_error() gives the text); nothing throws
 * across the ABI.  One handle == one HIP device + its workspaces; a handle is not thread-safe.
 * Separate handles may be driven from separate threads, but the handles of one process on one
 * device SHARE their HIP streams (a process-wide pool per device: main, second chunk stream, result
 * copy, H2D -- the runtime maps streams onto four hardware queues when they are created, and a
 * later handle's own streams could land two chunk streams on one queue): work of two handles
 * on one device serialises on those streams, ft8rx_sync / ft8rx_destroy of one waits for the
 * other's queued work, and ft8rx_set_profiling stage times include the other handle's kernels.
 * For independent concurrent decoding use one process per GPU (the multi-GPU path does).
 * All device workspaces are allocated at ft8rx_create(); the hot path allocates nothing.
 * Pointers are host pointers unless the parameter is named d_*.
 */
/* MAP OF THE ABI -- which entry points an adopter binds, and which exist for tests and measurements.
 *
 *   CORE (the drop-in boundary, SURVEY.md 8b: everything the Python surface of receiver.py / decoders.py needs)
 *     lifecycle        ft8rx_default_config  ft8rx_create  ft8rx_destroy  ft8rx_last_error  ft8rx_device_count  ft8rx_build_info  ft8rx_build_limits
 *     whole path       ft8rx_decode_batch  ft8rx_decode_messages                       (synchronous: host audio -> records / messages)
 *                      ft8rx_enqueue_batch  ft8rx_enqueue_batch_host  ft8rx_sync  ft8rx_fetch_results  ft8rx_fetch_results_view  (pipelined)
 *     host messages    ft8rx_package_batch  ft8rx_hashes_create / _destroy / _clear / _add / _size   (a14-a17: unpack, call hashes, dict fields)
 *     decoders.py      ft8rx_ldpc  ft8rx_osd  ft8rx_crc_valid  ft8rx_valid77                           (ldpc_decode, osd_012, crc_unpack91, unpack)
 *     streaming        ft8rx_hop_spectrum  ft8rx_sync_search                                       (AudioIn._callback, Receiver.search)
 *     multi-GPU        ft8rx_set_packed_output  ft8rx_packed_results  ft8rx_packed_output_fence  ft8rx_package_packed  ft8rx_alloc_host
 *                      ft8rx_free_host  ft8rx_d2h_async / _query / _event  ft8rx_device_pci_bus_id                                     (the gather of decoded messages)
 *   TUNING AND SERVICE (defaults are the measured best; results never depend on them)
 *     ft8rx_set_streams  ft8rx_set_subbatch  ft8rx_set_ladder_mode  ft8rx_set_ladder_grid  ft8rx_set_reject_log  ft8rx_staging_audio  ft8rx_copy_to_host
 *     ft8rx_results_to_device
 *   EXTENSIONS (no counterpart in the reference's receive path)
 *     ft8rx_synth_frames  ft8rx_synth_frames_ex                                        (f-1: workload generator)
 *     ft8rx_subtract  ft8rx_subtraction_list  ft8rx_encode_tones  ft8rx_merge_messages  ft8rx_set_search_mask   (f-4: subtraction passes)
 *     ft8rx_osd_ext                                                                    (order-3 / distance-gate knobs)
 *     ft8rx_set_msg_types  ft8rx_package_batch_ext  ft8rx_valid77_ext                  (opt-in message types)
 *     ft8rx_set_ap_calls  ft8rx_set_ap_max_hd  ft8rx_ap_patterns  ft8rx_ap_calls_probe (opt-in a-priori calls, ipass 7)
 *     ft8rx_set_recall  ft8rx_fetch_recall  ft8rx_set_recall_gates  ft8rx_recall_hypotheses  ft8rx_recall_probe  ft8rx_package_batch_recall
 *                                                                                      (opt-in recall of stations heard 30 s earlier, ipass 8)
 *     ft8rx_set_weak                                                                   (opt-in weak-signal sync)
 *     ft8rx_set_reports  ft8rx_fetch_reports  ft8rx_report_probe                       (opt-in measured SNR / frequency / time of each decode)
 *     ft8rx_ddc  ft8rx_ddc_host  ft8rx_ddc_taps                                        (down-converter: real / IQ input at 24 .. 192 kHz -> 12 kHz frames)
 *     ft8rx_ddc_stream_open  ft8rx_ddc_stream_push  ft8rx_ddc_stream_frame  ft8rx_ddc_stream_info  ft8rx_ddc_stream_read
 *     ft8rx_ddc_stream_close                                                           (the same on a continuous stream, state on the device)
 *     ft8rx_ddc_stream_frames                                                          (opt-in: 15-s or 7.5-s frames of chosen channels, live FT4)
 *     ft8rx_ddc_stream_grid_open  ft8rx_ddc_stream_grid_info  ft8rx_ddc_stream_grid_read  (opt-in spectrogram rows of every channel behind it)
 *     ft8rx_ddc_wide  ft8rx_ddc_wide_host  ft8rx_ddc_wide_taps  ft8rx_ddc_wide_plan     (pre-decimator: ONE stream at 240 kHz .. 129.6 MHz, 8- or
 *     ft8rx_ddc_wide_stream_open  ft8rx_ddc_wide_stream_push  ft8rx_ddc_wide_stream_read_mid   16-bit, in front of the down-converter)
 *     ft8rx_ddc_wide_stream_close
 *     ft8rx_ddc_rat  ft8rx_ddc_rat_host  ft8rx_ddc_rat_taps  ft8rx_ddc_rat_plan         (rational resampler: ONE stream at any other rate,
 *     ft8rx_ddc_rat_stream_open  ft8rx_ddc_rat_stream_push  ft8rx_ddc_rat_stream_read_mid      44.1 kHz, 2.048 MS/s, 10 MS/s ..., in front of
 *     ft8rx_ddc_rat_stream_close                                                       the down-converter)
 *     ft8rx_ft4_decode_batch  ft8rx_ft4_enqueue_batch  ft8rx_ft4_decode_messages  ft8rx_ft4_set  ft8rx_ft4_set_range  ft8rx_ft4_info
 *     ft8rx_ft4_subtract  ft8rx_ft4_subtraction_list  ft8rx_ft4_sub_info  ft8rx_ft4_staging_audio  ft8rx_ft4_encode_tones   (opt-in FT4, 7.5-s frames)
 *     ft8rx_ft4_report  ft8rx_ft4_report_info                                         (opt-in measured SNR / frequency / time of FT4 decodes)
 *     ft8rx_ft4_set_coherent  ft8rx_ft4_coh_info                                       (opt-in FT4 coherent LLRs: runs of two and four symbols)
 *     ft8rx_ft4_set_weak  ft8rx_ft4_weak_info                                          (opt-in FT4 weak search: coherent Costas sync, 2.6-Hz grid)
 *     ft8rx_ft4_set_coh_osd  ft8rx_ft4_coh_osd_info                                    (opt-in FT4 OSD on the coherent LLRs behind a whole-message score)
 *   TEST AND MEASUREMENT AIDS (stage entry points of the parity tests, timers, probes -- an adopter never calls these)
 *     ft8rx_spectrogram  ft8rx_sync_scores  ft8rx_llr_grid  ft8rx_cycle_spectrum  ft8rx_fine  ft8rx_get_fft_plans
 *     ft8rx_sync_scores_weak  ft8rx_fine_weak
 *     ft8rx_ft4_sync_weak
 *     ft8rx_ft4_grid  ft8rx_ft4_sync  ft8rx_ft4_demod  ft8rx_ft4_coherent  ft8rx_ft4_ldpc  ft8rx_ft4_osd  ft8rx_ft4_sub_probe
 *     ft8rx_ft4_verify
 *     ft8rx_set_profiling  ft8rx_get_stage_times  ft8rx_math_probe  (and the ft8rx_debug_* symbols of timing-only builds)
 *
 * LIMITS of this build against the reference's open-ended kwargs (pyft8_amd.receiver.config_from_kwargs names the kwarg when one is
 * exceeded; ft8rx_create answers -1): max_cands <= FT8RX_MAX_CANDS = 1024 (libft8rx.so) / 2048 (libft8rx_wide.so), more than the
 * build's search ranges have f0 bins, i.e. no limit (a larger max_cands keeps the same candidates; reference: any, default 200), search_time_range inside
 * [-36.4, +22.6] s (FT8RX_MIN_H0 / FT8RX_MAX_H0: beyond it the reference's own search raises IndexError), search_freq_range 12.5 .. 3000 Hz (libft8rx.so) / .. 5900 Hz
 * (libft8rx_wide.so), OSD flip counts <= 91 and <= 16384 trials.
 */
#ifndef FT8RX_H
#define FT8RX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FT8RX_NSAMP      180000   /* 15 s @ 12 kHz, int16 mono (receiver.py:9-12,241) */
#define FT8RX_GRID_ROWS  376      /* row 0 = never-written 1.0 row, rows 1..375 = hops (receiver.py:237-240) */
/* The spectrogram and cycle-spectrum layouts are compile-time widths.  The library is built twice from the same source:
 *   libft8rx.so       search_freq_range up to 3000 Hz, the reference's default (receiver.py:312): f0_hi <= 960
 *   libft8rx_wide.so  (-DFT8RX_WIDE) search_freq_range up to 5900 Hz: f0_hi <= 1888 -- twice the grid / spectrum memory per frame
 * Same ABI; ft8rx_build_info() tells which one is loaded.  Every f0 bin of the search range can pass sync_score_min (928 at the default
 * range, receiver.py:338-367), so max_cands may go up to the build's f0 bins (FT8RX_MAX_CANDS); the per-candidate workspaces are sized
 * at create time, per frame the smallest power of two >= max(max_cands, 256) candidate slots (256 at the default max_cands = 200).
 * (The reference allocates f0_hi + 16 grid columns, receiver.py:240, and
 * fails beyond ~5940 Hz, where the fine-sync slice runs off the 96001-bin cycle spectrum, receiver.py:181-182.) */
#ifdef FT8RX_WIDE
#define FT8RX_GRID_COLS  1920     /* bins 0..1919 of the 3840-point real FFT */
#define FT8RX_SPEC_BINS  96000    /* bins 0..95999 of the 192000-point real FFT */
#define FT8RX_MAX_F0     1888
#define FT8RX_MAX_CANDS  2048     /* upper bound for config.max_cands: the keys k_topk sorts */
#else
#define FT8RX_GRID_COLS  976      /* receiver.py:240 at the default range: 960 + 16 */
#define FT8RX_SPEC_BINS  49152    /* kept bins of the 192000-point cycle spectrum (receiver.py:280-286) */
#define FT8RX_MAX_F0     960
#define FT8RX_MAX_CANDS  1024     /* upper bound for config.max_cands: the keys k_topk sorts (the reference's default is 200, receiver.py:311) */
#endif
#define FT8RX_MIN_H0     (-898)   /* bounds of config.h0_lo / h0_hi (search_time_range -36.4 .. +22.6 s; the reference's default is -2 .. +3 s): where the   */
#define FT8RX_MAX_H0     578      /* reference's own search stops indexing its 750-row grid (rows h0 + 148 .. h0 + 172, receiver.py:322, 346-347)            */
#define FT8RX_MIN_H0_FD  (-140)   /* candidates with h0 in [MIN_H0_FD, MAX_H0_FD] (-6.1 .. +8.3 s): the middle Costas block of every tweak lies inside the      */
#define FT8RX_MAX_H0_FD  220      /* 3200-sample fine-sync series and the frequency-domain scores / grid apply; further out the reads are clamped (:189-195)   */
                                  /* and the candidate is scored in the time domain, one series per tweak (kernels/fine_sync.hpp: k_fine_td)                 */
#define FT8RX_EVENT_CAP  512      /* per-frame capacity of the CRC-pass event log */

/* Receiver(...) kwargs (receiver.py:311-313) + module/decoder constants (receiver.py:30,78,91,95;
 * decoders.py:223).  BASELINE "30 iters / OSD depth" extension knobs are these same fields. */
typedef struct {
    float   sync_score_min;          /* 85 */
    int32_t max_cands;               /* 200 */
    int32_t f0_lo, f0_hi;            /* 32, 960 = int(search_freq_range / 3.125) */
    int32_t h0_lo, h0_hi;            /* -37, 87 = int((search_time_range + 0.5) * 25) */
    int32_t bp_nc0_a, bp_iters_a;    /* 35, 5  : ldpc_decode(llr, 35, 5)  (ipass 0 and 3) */
    int32_t bp_nc0_b, bp_iters_b;    /* 90, 20 : ldpc_decode(llr, 90, 20) (ipass 4) */
    int32_t osd_single, osd_double;  /* 30, 2  : osd_012(llr, 30, 2) */
    float   llr_sd_min;              /* 5 : Candidate.llr_sd_min */
    /* Extension knobs with no reference counterpart (BASELINE config 4 "OSD depth-3"); 0 = off = the reference's osd_012. */
    int32_t osd_triple;              /* 0 : order-3 reprocessing -- after the reference's trials, triple flips (i, j, k), k < j < i < osd_triple
                                      *     over the least reliable basis positions, i-major; C(osd_triple, 3) extra trials (<= 40) */
    int32_t osd_max_hd;              /* 0 : acceptance gate -- an OSD trial counts (and calls unpack) only if its 174-bit codeword differs from
                                      *     the hard decisions in <= osd_max_hd positions.  The reference accepts the first CRC-valid trial
                                      *     whatever its distance (decoders.py:248-272), which is where its false decodes come from. */
} ft8rx_config;

/* Opt-in message types (extension; ft8rx_set_msg_types): FT8RX_MT_* bits, i3.n3 of the 77-bit word (Franke, Somerville, Taylor,
 * QEX 2020).  The reference leaves them unimplemented (decoders.py:16-49 returns None); 0 = its rule, bit for bit. */
#define FT8RX_MT_FREE_TEXT   1        /* 0.0  13 characters of a 42-character alphabet */
#define FT8RX_MT_DXPEDITION  2        /* 0.1  c28 c28 h10 r5 */
#define FT8RX_MT_FIELD_DAY   4        /* 0.3 / 0.4  c28 c28 R1 n4 k3 s7 */
#define FT8RX_MT_TELEMETRY   8        /* 0.5  71 bits, 18 hex digits */
#define FT8RX_MT_RTTY_RU     16       /* 3    t1 c28 c28 R1 r3 s13 */
#define FT8RX_MT_EU_VHF      32       /* 5    h12 h22 R1 r3 s11 g25 */
#define FT8RX_MT_ALL         63

enum { FT8RX_ST_ACTIVE = 0, FT8RX_ST_DECODED = 1, FT8RX_ST_STOP_GRID_SD = 2, FT8RX_ST_STOP_COSTAS = 3,
       FT8RX_ST_STOP_FINE_SD = 4, FT8RX_ST_EXHAUSTED = 5 };
enum { FT8RX_M_GOOD91 = 0, FT8RX_M_LDPC_A = 1, FT8RX_M_LDPC_B = 2, FT8RX_M_OSD = 3, FT8RX_M_LDPC_B_OSD = 4,
       FT8RX_M_AP_CODEWORD = 5 /* ipass 7, full pattern: codeword test (ft8rx_set_ap_calls) */,
       FT8RX_M_RECALL = 6      /* ipass 8: hypothesis test of a recall entry (ft8rx_set_recall) */ };

/* One candidate's outcome (replaces the state of a reference `Candidate`, receiver.py:29-66). 48 bytes. */
typedef struct {
    uint64_t msg_lo, msg_hi;         /* 77-bit payload, bit 76 = first transmitted bit; valid iff status==DECODED */
    float    score, grid_sd, fine_sd;
    int16_t  f0_idx, h0_idx;
    int8_t   ttweak, ftweak, snr_grid, snr_fine;
    uint8_t  status, ipass, ap, method;  /* ipass 7 / ap 5..10: the opt-in a-priori step of ft8rx_set_ap_calls */
    int16_t  n_its;                  /* BP iteration index or OSD trial index of the success */
    uint8_t  nsync;
    uint8_t  osd_hd;                 /* OSD decodes: Hamming distance of the accepted codeword to the 174 hard decisions;
                                      * ipass 7: the same distance to the hard decisions of the un-overridden fine LLRs */
    uint32_t pad2;
} ft8rx_record;

/* One CRC-14-passing, non-zero 77-bit word met on the decode ladder (= one call of the reference's
 * unpack(), decoders.py:131).  The host replays these in reference order to reproduce the call-hash
 * table side effects (databases.py:10-26).  24 bytes. */
typedef struct {
    uint64_t msg_lo, msg_hi;
    uint16_t cand;                   /* candidate index within the frame */
    uint8_t  ipass;                  /* ladder step the call belongs to (0..6; 7 = ft8rx_set_ap_calls) */
    uint8_t  slot;                   /* attempt index inside the ipass step (AP index / saved-llr index; ipass 7: 2 * ap for BP and
                                      * the codeword test, 2 * ap + 1 for OSD) */
    uint16_t seq;                    /* order inside the attempt: GOOD91=0, BP iteration+1, OSD trial */
    uint16_t valid;                  /* unpack() would have returned a tuple */
} ft8rx_event;

/* One emitted message (the argument of the reference's on_message callback, receiver.py:61-65, before string
 * formatting).  64 bytes. */
typedef struct {
    char     f[3][16];               /* msg_tuple */
    int16_t  cand, f0_idx, h0_idx;
    int8_t   snr, ttweak, ftweak;
    uint8_t  ipass, ap, method, fine;
    uint8_t  pad[3];
} ft8rx_message;

/* The same for a handle with msg_types != 0 (ft8rx_package_batch_ext): fields wide enough for every message type, and the
 * type.  f[0..2] = msg_tuple: (first call -- or "TU; call", or "call RR73;" for DXpedition --, second call, the rest); free text and
 * telemetry are (text, "", "").  112 bytes. */
typedef struct {
    char     f[3][32];               /* msg_tuple, NUL-terminated */
    int16_t  cand, f0_idx, h0_idx;
    int8_t   snr, ttweak, ftweak;
    uint8_t  ipass, ap, method, fine;
    uint8_t  i3, n3;                 /* message type: i3, and n3 when i3 == 0 (0 otherwise) */
    uint8_t  pad[1];
} ft8rx_message_ext;

typedef struct ft8rx_handle ft8rx_handle;
typedef struct ft8rx_hashes ft8rx_hashes;                           /* persistent call-hash table, ft8rx_hashes_* below */

/* ---- lifecycle -------------------------------------------------------------------------- */
int  ft8rx_default_config(ft8rx_config* cfg);                       /* Receiver.__init__ defaults */
int  ft8rx_create(const ft8rx_config* cfg, int device, int max_frames, ft8rx_handle** out);
void ft8rx_destroy(ft8rx_handle* h);
const char* ft8rx_last_error(ft8rx_handle* h);                      /* h may be NULL: last create error */
int  ft8rx_device_count(void);
/* PCI address of a device ("0000:c1:00.0"; buf >= 16 bytes): lets a multi-rank host place each rank's threads and page-locked
 * buffers on the GPU's NUMA node (/sys/bus/pci/devices/<address>/numa_node), as bench.py does */
int  ft8rx_device_pci_bus_id(int device, char* buf, int len);
/* the compile-time widths of the loaded library (FT8RX_GRID_COLS, FT8RX_SPEC_BINS, FT8RX_MAX_F0): 976 / 49152 / 960, or
 * 1920 / 96000 / 1888 for the wide build */
int  ft8rx_build_info(int32_t* grid_cols, int32_t* spec_bins, int32_t* max_f0);
/* ... and its capacities (FT8RX_MAX_CANDS, FT8RX_EVENT_CAP): 1024 / 512, or 2048 / 512 for the wide build */
int  ft8rx_build_limits(int32_t* max_cands, int32_t* event_cap);
/* FFT radix plans the kernels use (0-terminated, <= 8 entries each): 1920, 3200, 300, 320 point */
int  ft8rx_get_fft_plans(int32_t* p1920, int32_t* p3200, int32_t* p300, int32_t* p320);

/* ---- whole hot path: audio -> candidate records ------------------------------------------
 * Stands in for AudioIn._callback x375 + Receiver.search + the Candidate.decode ladder driven by
 * Receiver.manage_cycle (receiver.py:295-306, 338-367, 68-107, 389-398) under frame-complete
 * semantics, for n_frames independent 15-s frames.
 *   records : [n_frames][cfg.max_cands]   counts : [n_frames]
 *   events  : [n_frames][FT8RX_EVENT_CAP] event_counts : [n_frames] (may exceed the cap => truncated) */
int  ft8rx_decode_batch(ft8rx_handle* h, const int16_t* audio, int n_frames,
                        ft8rx_record* records, int32_t* counts, ft8rx_event* events, int32_t* event_counts);
/* Same, split for pipelining: audio already resident in HBM (device pointer); enqueue is asynchronous.  Results are double
 * buffered: when a batch's kernels finish, a copy stream moves its records/events into page-locked host buffers while the next
 * enqueued batch computes.  ft8rx_fetch_results waits for and returns the OLDEST unfetched batch (or the latest batch again if
 * all have been fetched); at most two batches are retained -- a third enqueue drops the oldest.  Steady state:
 *   enqueue(0); for k = 1..: enqueue(k); fetch(k-1); <host message layer of k-1>   -- the GPU never waits for the host. */
int  ft8rx_enqueue_batch(ft8rx_handle* h, const int16_t* d_audio, int n_frames);
/* Ordering: consecutive enqueued batches of the same size run as free-running chunk streams (chunk i of batch k+1 follows chunk i of
 * batch k on its own HIP stream, no per-batch fork / join; only the result copy waits for all chunks).  Every other entry point of
 * the handle -- stage functions, ft8rx_decode_batch, ft8rx_subtract, profiling passes -- first waits until the batches in flight are
 * complete, so mixing them with enqueue / fetch is safe (and costs that wait). */
/* The same pipeline fed from HOST memory: the audio of batch k+1 is copied (in chunks, on a dedicated stream, into the second of two
 * device staging buffers) while batch k computes, so in steady state  enqueue_host(k+1); fetch(k); <host layer of k>  hides the PCIe
 * transfer behind the kernels.  `audio` must stay valid until the batch has been fetched; page-locked memory (ft8rx_alloc_host) makes
 * the copies truly asynchronous. */
int  ft8rx_enqueue_batch_host(ft8rx_handle* h, const int16_t* audio, int n_frames);
/* ---- float32 frames (opt-in) ------------------------------------------------------------------------------
 * The _f32 entries take the frames as [n_frames][180000] float32 instead of int16 and are otherwise their twins: the same plan,
 * chunks, result slots, streams, results and refusals.  Only the two kernels that read audio differ (k_spectrogram_f32, k_cyc_a_f32):
 * they use the samples as they are where the int16 kernels convert, so integer-valued floats in the int16 range give the int16
 * entries' results byte for byte, and everything behind the dB grid and the cycle spectrum works on level differences and normalised
 * quantities: scaling a frame by a power of two shifts its grid by 20 log10 of the factor and changes no message.  The level is the
 * caller's: no gain has to be chosen and nothing is rounded.  Non-finite samples are the caller's business: they are not looked for
 * on the device, and a NaN or infinity poisons its own frame only, since every workspace is indexed by frame.
 * Device frames (ft8rx_enqueue_batch_f32) are aligned to 8 bytes, a pair of samples.  The float staging audio
 * (ft8rx_staging_audio_f32, 720 000 bytes per frame, and the second buffer of ft8rx_enqueue_batch_host_f32) is allocated on first use. */
int  ft8rx_decode_batch_f32(ft8rx_handle* h, const float* audio, int n_frames,
                            ft8rx_record* records, int32_t* counts, ft8rx_event* events, int32_t* event_counts);   /* ft8rx_decode_batch */
int  ft8rx_enqueue_batch_f32(ft8rx_handle* h, const float* d_audio, int n_frames);                                  /* ft8rx_enqueue_batch */
int  ft8rx_enqueue_batch_host_f32(ft8rx_handle* h, const float* audio, int n_frames);                               /* ft8rx_enqueue_batch_host */
int  ft8rx_sync(ft8rx_handle* h);
int  ft8rx_fetch_results(ft8rx_handle* h, int n_frames, ft8rx_record* records, int32_t* counts,
                         ft8rx_event* events, int32_t* event_counts);
/* Only events[f][0 .. min(event_counts[f], FT8RX_EVENT_CAP)) are written / valid -- here, in the view below and in
 * ft8rx_decode_batch; the rest of a frame's row is left as it was.  For batches whose event log exceeds 1 MB the GPU packs the used
 * entries (the log is 12 KB per frame, a tenth of it used) straight into page-locked host memory: eight ranks sharing the host
 * links move ~8 MB instead of 100 MB per 8192-frame shard. */
/* Zero-copy variant of ft8rx_fetch_results: waits for the same batch and returns pointers INTO the handle's page-locked result
 * buffers (records packed [n_frames][cfg.max_cands], events [n_frames][FT8RX_EVENT_CAP]).  They stay valid until two more
 * batches have been enqueued (the slot is then reused). */
int  ft8rx_fetch_results_view(ft8rx_handle* h, int n_frames, const ft8rx_record** records, const int32_t** counts,
                              const ft8rx_event** events, const int32_t** event_counts);
/* Multi-GPU gather support: copies the LATEST batch's results, device to device, into caller-owned device buffers laid out like
 * the host outputs of ft8rx_decode_batch (records packed [n_frames][cfg.max_cands]); waits for the batch first.  The caller hands
 * these buffers to its collective (RCCL gather over xGMI, pyft8_amd/distributed.py) -- no host round trip.  Any pointer may be NULL. */
int  ft8rx_results_to_device(ft8rx_handle* h, int n_frames, ft8rx_record* d_records, int32_t* d_counts,
                             ft8rx_event* d_events, int32_t* d_event_counts);
/* ---- packed results: what a multi-GPU gather moves (the reference has no counterpart) -------------------------
 * The dense result arrays are [n_frames][max_cands] records + [n_frames][512] events = up to 24 KB per frame, of which the host
 * message layer reads ~4 KB: the records of the candidates that DECODED or made at least one unpack() call (an event), and the
 * used part of the event log.  With a packed output set, every enqueued batch ends with three small kernels that write exactly
 * that, back to back, into the caller's buffer of the batch's result slot:
 *     ft8rx_packed_header | ft8rx_packed_frame[n_frames] | ft8rx_record[n_records] | ft8rx_event[n_events]
 * frame f's records are records[rec_off .. rec_off + n_rec) in candidate order, each with pad2 = its candidate index inside the
 * frame; its events are events[ev_off .. ev_off + min(n_ev, FT8RX_EVENT_CAP)).  ft8rx_package_packed renders the same messages from
 * this as ft8rx_package_batch does from the dense arrays (the replay only ever looks at those candidates), so a rank sends ~4 KB
 * per frame to rank 0 instead of 13-24 KB and rank 0 keeps the packed form (pyft8_amd/distributed.py: PackedGather). */
#define FT8RX_PACKED_MAGIC 0x50385446u      /* "FT8P" */
typedef struct {
    uint32_t magic;                  /* FT8RX_PACKED_MAGIC */
    int32_t  n_frames;
    int32_t  n_records, n_events;    /* totals over the batch */
    uint64_t bytes;                  /* header + frame table + records + events */
    int32_t  max_cands;              /* cfg.max_cands of the producing handle */
    int32_t  overflow;               /* != 0: `bytes` exceeds the buffer's capacity -- only header and frame table were written */
} ft8rx_packed_header;               /* 32 bytes */
typedef struct {
    int32_t  rec_off, ev_off;        /* first record / event of the frame in the packed runs */
    uint16_t n_cand;                 /* the frame's candidate count (counts[f] of the dense form) */
    uint16_t n_rec;                  /* records kept: decoded or with at least one event */
    int32_t  n_ev;                   /* event_counts[f] of the dense form (may exceed FT8RX_EVENT_CAP: the log overflowed) */
} ft8rx_packed_frame;                /* 16 bytes */
/* d_buf0 / d_buf1: one buffer per result slot (batches alternate), cap_bytes each, device memory or page-locked host memory
 * (ft8rx_alloc_host: the kernels then write straight across PCIe); NULL, NULL turns the packed output off.  Worst case per frame:
 * 16 + 48 max_cands + 24 x 512 bytes; config 1 frames need ~4 KB.  Applies to batches enqueued afterwards. */
int  ft8rx_set_packed_output(ft8rx_handle* h, void* d_buf0, void* d_buf1, uint64_t cap_bytes);
/* The packed output of the batch the last ft8rx_fetch_results / _view / ft8rx_decode_batch call returned (that call has waited for
 * it): which of the two buffers (0 / 1) and a copy of its header.  -1 if no packed output was set when that batch was enqueued. */
int  ft8rx_packed_results(ft8rx_handle* h, int32_t* which, ft8rx_packed_header* header);
/* A consumer that reads packed buffer `which` (0 / 1) ASYNCHRONOUSLY on a stream of its own (an RCCL send) hands over a HIP event
 * (hipEvent_t) recorded on that stream behind its last read: the next batch that packs into this buffer -- two enqueues later --
 * makes its pack kernels wait for the event on the device.  One pending fence per buffer; the event must stay alive until that
 * batch has been enqueued.  NULL clears it. */
int  ft8rx_packed_output_fence(ft8rx_handle* h, int which, void* hip_event);
/* Host side (no GPU needed): messages of frames [frame_lo, frame_lo + n_frames) of a packed buffer, as ft8rx_package_batch renders
 * them from the dense arrays (n_threads / table / flags as there); out [n_frames][max_msgs].  Returns -1 for a malformed or
 * overflowed buffer. */
int  ft8rx_package_packed(const void* packed, uint64_t bytes, int frame_lo, int n_frames, ft8rx_message* out, int max_msgs,
                          int32_t* out_counts, int n_threads, ft8rx_hashes* table, int32_t* flags);
/* per-kernel HIP-event timing of the most recent enqueue (enable before enqueue). names/ms: up to 16 */
/* number of HIP streams a batch is cut across (1..8, default 2: measured best, profiles/archive/r02_notes.md); profiling mode always uses one */
int  ft8rx_set_streams(ft8rx_handle* h, int n);
/* frames per kernel chain inside a stream's share of a batch (default FT8RX_SUBBATCH_DEFAULT; 0 = the whole share in one chain): a
 * large batch runs as a sequence of cache-sized sub-batches, each through the whole path before the next starts, so that a stage
 * reads what the stage before it wrote from L2 / MALL instead of HBM.  Records, events and messages do not depend on it. */
#define FT8RX_SUBBATCH_DEFAULT 256    /* measured: 128 .. 256 are equal on dense frames (BASELINE configs 2, 3), 256 is 10 % better on sparse ones (config 4) */
int  ft8rx_set_subbatch(ft8rx_handle* h, int frames);
/* how the fine-stage BP attempts of a batch are launched; records and messages are identical either way:
 * 0 (default) = in the reference's ladder order (receiver.py:84-98) as three launches, candidates that are decided dropping out in
 *     between -- least work, highest throughput;
 * 1 = all five AP variants in one launch -- one dependent BP instead of three: lower latency for batches too small to fill the GPU
 *     (one frame: 0.38 vs 0.49 ms host to host).  The event log then also holds CRC-passing words of attempts the ladder would not
 *     have reached; ft8rx_package_batch skips them. */
int  ft8rx_set_ladder_mode(ft8rx_handle* h, int mode);
/* Test and tuning seam: the most blocks a ladder kernel is launched with.  Every ladder kernel (ipass-0 and a-priori BP, fine sync,
 * OSD, reports) runs min(items possible, cap) blocks that stride over a device work list; the compiled cap (32768 blocks) gives
 * nearly every block one item at most, a small cap makes every block walk many.  cap = 0 restores the compiled default, 1 .. 32768
 * is taken, anything else is refused; the NaN kernels of OSD run min(512, cap) blocks (also behind ft8rx_osd / ft8rx_osd_ext, whose main kernel keeps one block per vector).  Waits for the batches in flight, then holds
 * for every later launch.  Records, events and messages do not depend on it (tests/test_gpu_ladder_stride.py). */
int  ft8rx_set_ladder_grid(ft8rx_handle* h, int cap);
/* Opt-in message types (FT8RX_MT_* bits; 0 = the default = the reference's rule): with a bit set, a CRC-valid word of that type that
 * passes its plausibility gate (csrc/ft8_dev.h: ft8_valid77_ext) stops a candidate's ladder like any other message; free text and
 * telemetry are never accepted from an OSD trial.  Records / events are then packaged with
 * ft8rx_package_batch_ext; ft8rx_decode_messages and the packed output (ft8rx_set_packed_output) refuse a non-zero mask.  Applies to
 * batches enqueued afterwards.  A handle setting rather than a field of ft8rx_config, whose layout callers' bindings hard-code. */
int  ft8rx_set_msg_types(ft8rx_handle* h, int32_t mask);
/* Opt-in weak-signal sync (extension).  on != 0 changes three stages of the batches enqueued afterwards:
 *   search   the Costas score summed over all three blocks (k_sync3), kept above sync_min instead of config.sync_score_min;
 *   fine     a joint scan of ftweak -56 .. +56 (step 8, +-3.5 Hz) x ttweak -16 .. +16 (step 2) scored on all three blocks (k_fine_weak);
 *   gates    no llr_sd_min stop at grid or fine -- the Costas gate (>= 7 of 21) is the only stop before the decoders -- and every OSD
 *            trial (ipass 5, 6) counts only within osd_max_hd of the hard decisions (config.osd_max_hd, when non-zero, wins).
 * The ladder, BP, OSD, the LLR arithmetic and the message layer are unchanged; records keep their layout (ttweak / ftweak now span
 * -16 .. 16 / -56 .. 56).  on = 0 restores the reference's stages (sync_min and osd_max_hd are then ignored).  Only writes host state,
 * allocates nothing; batches in flight keep the setting they were enqueued with.  Refused together with msg_types != 0,
 * ft8rx_set_ap_calls, ft8rx_set_recall and the packed output.  sync_min > 0, osd_max_hd 1 .. 174. */
#define FT8RX_WEAK_SYNC_MIN_DEFAULT 148.5f
#define FT8RX_WEAK_OSD_MAX_HD_DEFAULT 30
int  ft8rx_set_weak(ft8rx_handle* h, int32_t on, float sync_min, int32_t osd_max_hd);
/* Opt-in a-priori decoding with the operator's own call and the DX station's call (extension).  NULL or ""
 * = unset; both unset (the default) = the reference's ladder, same kernels and launches.  With a call set, a candidate the whole
 * reference ladder left undecoded after the fine stage (status EXHAUSTED) gets ipass 7: the patterns whose calls are set --
 * ap 5 "MY ???", 6 "MY DX ???", 7 "CQ DX ???" (known bits forced to +-5, BP_B then OSD) and 8 "MY DX RRR", 9 "MY DX 73",
 * 10 "MY DX RR73" (a codeword test) -- accepted only if the codeword lies within ap_max_hd of the hard decisions of the
 * un-overridden fine LLRs; the smallest distance wins (ties: pattern order).  Every record ipass 0..6 decodes is unchanged.  Only
 * standard callsigns (3..6 letters / digits, the c28 form of i3 = 1 messages); anything else returns -1 naming the argument.
 * Applies to batches enqueued afterwards and allocates nothing (cheap to call every cycle).  Refused with msg_types != 0 and with
 * the packed output (ft8rx_set_packed_output). */
#define FT8RX_AP_MAX_HD_DEFAULT 36
int  ft8rx_set_ap_calls(ft8rx_handle* h, const char* my_call, const char* dx_call);
/* the ipass-7 acceptance gate (1..174; default FT8RX_AP_MAX_HD_DEFAULT) */
int  ft8rx_set_ap_max_hd(ft8rx_handle* h, int32_t max_hd);
/* Host only (tests): the six patterns ap 5..10 of (my_call, dx_call) as [6][174] bytes in LLR order -- bits_out the known values
 * (full patterns: the 174-bit codeword), mask_out which positions are known (0 for a pattern whose calls are unset).  -1 for
 * a call that is not a standard callsign (ft8rx_last_error(NULL)). */
int  ft8rx_ap_patterns(const char* my_call, const char* dx_call, uint8_t* bits_out, uint8_t* mask_out);
/* Test entry: ipass 7 alone, with the handle's setting, on n <= cfg.max_cands fine-LLR vectors [n][174] taken as the candidates
 * 0 .. n - 1 of one frame that the reference's ladder left undecoded -- the batch's own launch sequence.  -> their records (ipass 7
 * and ap / method / osd_hd where a pattern was accepted, status EXHAUSTED otherwise) and the frame's event log (events: FT8RX_EVENT_CAP
 * entries; *event_count may exceed that).  -1 while no call is set. */
int  ft8rx_ap_calls_probe(ft8rx_handle* h, const float* llr, int n, ft8rx_record* records, ft8rx_event* events, int32_t* event_count);
/* Opt-in recall decoding (extension): ipass 8.  A recall entry is a message the same stream decoded two cycles
 * (30 s) earlier, with its grid position.  For every entry the next batch runs a forced fine sync at (f0_idx, h0_idx) -- the tweak
 * scan runs; the sync threshold, the Costas gate and llr_sd_min are not applied -- and tests the entry's likely continuations against
 * the LLRs of that grid: for "A B X" (A a standard call) the word itself, A B RRR / RR73 / 73, A B -30 .. +30, A B R-30 .. R+30 (the
 * repeat's duplicate dropped; at most 126); for "CQ / QRZ / DE B X" the word itself.  The hypothesis whose codeword has the smallest
 * soft distance D = sum |llr| over the disagreeing positions wins (ties: list order); it is accepted iff its Hamming distance hd to
 * the hard decisions is <= max_hd and the runner-up's hd exceeds it by >= min_gap (no runner-up: hd 174).
 * Only i3 = 1 / 2 words whose second call is a standard call and whose first is a standard call or a DE / QRZ / CQ token qualify;
 * others are skipped.  An entry is also skipped when a ladder record of its frame is DECODED within +-2 f0 bins and +-4 h0 rows.
 * The ladder's records, counts and events do not change: results go to a separate area, ft8rx_fetch_recall. */
#define FT8RX_RECALL_MAX 64                  /* entries per frame */
#define FT8RX_RECALL_MAX_HD_DEFAULT 46
#define FT8RX_RECALL_MIN_GAP_DEFAULT 12
typedef struct {                             /* 24 bytes */
    uint64_t msg_lo, msg_hi;                 /* the 77-bit word, as ft8rx_record holds it */
    int16_t  f0_idx, h0_idx;                 /* its grid position (the record's) */
    int8_t   ttweak, ftweak;                 /* its fine tweaks (informative: the forced fine sync scans its own) */
    uint16_t pad;                            /* 0 */
} ft8rx_recall_entry;
/* entries [n_frames][FT8RX_RECALL_MAX] (row f: counts[f] <= FT8RX_RECALL_MAX entries of frame f of the next batch), consumed by the
 * next enqueue (ft8rx_enqueue_batch*, ft8rx_decode_batch), like ft8rx_set_search_mask; the batch must have exactly n_frames frames.
 * Waits for the batches in flight.  NULL / n_frames = 0 clears a pending setting.  Positions outside the configured search range are
 * refused.  Refused with msg_types != 0 and on the packed output; ft8rx_decode_messages refuses a pending setting. */
int  ft8rx_set_recall(ft8rx_handle* h, const ft8rx_recall_entry* entries, const int32_t* counts, int n_frames);
/* the recall results of the batch the last ft8rx_fetch_results / ft8rx_decode_batch handed out: records [n_frames][FT8RX_RECALL_MAX]
 * (record e = entry e: ipass 8, method FT8RX_M_RECALL, status DECODED (accepted) or EXHAUSTED (tested, rejected), ap = the
 * hypothesis class 0 repeat / 1 RRR / 2 RR73 / 3 73 / 4 report / 5 R-report, n_its = its index in the list, osd_hd = its hd,
 * pad2 = the runner-up's hd, score / grid_sd = the two soft distances (grid_sd -1: no runner-up), fine_sd / snr_fine of the grid's
 * LLRs, ttweak / ftweak / nsync of the forced fine sync; a skipped entry's record stays zero) and counts [n_frames] (0 for a batch
 * enqueued without entries). */
int  ft8rx_fetch_recall(ft8rx_handle* h, int n_frames, ft8rx_record* records, int32_t* counts);
/* max_hd 1..174, min_gap 0..174; applies to batches enqueued afterwards */
int  ft8rx_set_recall_gates(ft8rx_handle* h, int32_t max_hd, int32_t min_gap);
/* Host only (tests): the hypothesis list of one entry -> its length (0: the entry does not qualify), words [126] */
int  ft8rx_recall_hypotheses(const ft8rx_recall_entry* entry, uint64_t* words_lo, uint64_t* words_hi);
/* Test entry: k_recall_score alone on caller-supplied fine grids sgrid [n][79][8] (magnitudes, ft8rx_fine's sgrid) for entries [n]
 * (no skip rule, tweaks 0) -> records [n] as ft8rx_fetch_recall gives them. */
int  ft8rx_recall_probe(ft8rx_handle* h, const float* sgrid, const ft8rx_recall_entry* entries, int n, ft8rx_record* records);
/* ft8rx_package_batch plus each frame's recall results (ft8rx_fetch_recall: recall [n_frames][FT8RX_RECALL_MAX], recall_counts): after
 * all of a frame's ladder messages, the accepted ones in entry order (cand = the entry index, ipass 8), unless the frame has emitted
 * the same text already; each updates the call-hash table as a ladder decode of the word does.  No GPU needed. */
int  ft8rx_package_batch_recall(const ft8rx_record* records, const int32_t* counts, const ft8rx_event* events, const int32_t* event_counts,
                                const ft8rx_record* recall, const int32_t* recall_counts, int n_frames, int max_cands, ft8rx_message* out,
                                int max_msgs, int32_t* out_counts, int n_threads, ft8rx_hashes* table, int32_t* flags);
/* Opt-in measured signal reports (extension).  A record's snr_grid / snr_fine and its position are the
 * reference's quantities: the spread of the payload grid, and the search-grid position plus the tweaks.  With the setting on, every
 * record that ends a batch's chain DECODED (ipass 0 .. 6, and 7 with ft8rx_set_ap_calls) is measured once more with its own 79 tones
 * (word -> CRC-14 -> LDPC -> Gray map, Costas blocks) on the series of its slice, fb = 50 f0_idx + ftweak:
 *   P(tau, delta) = sum_s |sum_{n<32} z[tau + 32 s + n] e^{-2 pi i n (tone_s + delta) / 32}|^2,  samples outside [0, 3200) = 0,
 *   tau = tb - 28 .. tb + 12 (tb = 8 h0_idx + (h0_idx < 0) + ttweak, 5-ms samples), delta = -0.7, -0.6 .. +0.7 tone spacings;
 *   the first maximum in tau-major order, moved on each axis where it is interior by the three-point parabola (on a border: no shift
 *   and an EDGE flag);  f_hz = 0.0625 fb + 6.25 delta,  t_sec = 0.005 tau;
 *   snr_db = 10 log10(max(on / off - 1, 1e-3) * 6.25 / 2500) at the peak's integer tau and the interpolated delta: on = the mean over
 *   the symbols of the rectangular |DFT|^2 at the symbol's tone, off = median / ln 2 * 32 / sum w^2 of the Hann-weighted cells
 *   (w[n] = 1/2 - 1/2 cos(2 pi (n + 1/2) / 32), all 8 tones) more than two tones from the tone of the symbol, of the one before and of
 *   the one after; when on / off > 300, of those cells of the tones 0 .. 5 only (a strong signal leaks into the two cells next to the
 *   edge of the slice).  dB in 2500 Hz, the convention of the workload generator.
 * A record whose h0_idx lies outside [FT8RX_MIN_H0_FD, FT8RX_MAX_H0_FD] or whose slice fb - 150 .. fb + 849 leaves the spectrum gets
 * FT8RX_RP_INVALID and NaN fields.  Records, counts and events do not change; off (the default), nothing is launched or allocated.
 * Recall records (ipass 8) get no report.  Refused together with the packed output (ft8rx_set_packed_output). */
#define FT8RX_RP_MEASURED 1u          /* the slot's record was DECODED and a report was made (flags = 0: no report) */
#define FT8RX_RP_INVALID  2u          /* ... but it could not be measured: the fields are NaN */
#define FT8RX_RP_EDGE_T   4u          /* the peak lies on the border of the tau window: t_sec is not interpolated */
#define FT8RX_RP_EDGE_F   8u          /* the peak lies on the border of the delta window: f_hz is not interpolated */
typedef struct {                      /* 24 bytes */
    float    snr_db;                  /* dB in 2500 Hz */
    float    f_hz;                    /* frequency of tone 0 */
    float    t_sec;                   /* start of symbol 0 in the frame */
    float    score;                   /* P at the peak */
    uint32_t flags;                   /* FT8RX_RP_* */
    uint32_t pad;                     /* 0 */
} ft8rx_report;
/* on != 0: batches enqueued afterwards end with the measurement step (the first call allocates the report arrays of both result
 * slots); 0: back to the default.  Waits for the batches in flight. */
int  ft8rx_set_reports(ft8rx_handle* h, int32_t on);
/* the reports of the batch the last ft8rx_fetch_results / ft8rx_decode_batch handed out: reports [n_frames][cfg.max_cands], indexed like
 * its records (all zero for a batch enqueued with the setting off). */
int  ft8rx_fetch_reports(ft8rx_handle* h, int n_frames, ft8rx_report* reports);
/* Test entry: the measurement step alone -- the batch's own launch sequence -- on caller-supplied cycle spectra spec
 * [n_frames][FT8RX_SPEC_BINS] complex64 for n candidates (frame, f0_idx, h0_idx, ttweak, ftweak, word), at most the handle's candidate
 * stride per frame -> reports [n].  Needs no ft8rx_set_reports. */
int  ft8rx_report_probe(ft8rx_handle* h, const float* spec, int n_frames, int n, const int32_t* frame, const int32_t* f0_idx,
                        const int32_t* h0_idx, const int32_t* ttweak, const int32_t* ftweak, const uint64_t* msg_lo, const uint64_t* msg_hi,
                        ft8rx_report* reports);
/* Down-converter (extension): n_streams sample arrays of one kind at rate_hz = 12000 D, D = 1, 2, 4, 8, 16 (real
 * int16 at D = 1 is a frame already and is refused), each n_samples <= 180000 D long (zero before sample 0 and after the last) ->
 * n_out frames of 180000 int16 at 12 kHz.  Output j is the USB audio of stream src[j] with the dial f_dial_hz[j] Hz from the stream's
 * centre (a real stream's centre is 0 Hz; any value in [-rate/2, rate/2), the spectrum wraps; outputs may share a stream):
 *   mixer    fc = f_dial + 3000, w = round(fc / rate 2^32) mod 2^32, phase of input sample n = (w n mod 2^32) / 2^32 cycles;
 *   filters  Kaiser-windowed sincs, zero phase: rate -> 24 kHz (D >= 4: 17 / 31 / 61 taps), then 24 -> 12 kHz (283 taps; 143 at D = 1,
 *            where nothing is decimated); ft8rx_ddc_taps hands out the float32 taps;
 *   audio    y[m] = gain g Re(i^m z[m]), g = 1 for IQ and 2 for real kinds: unit gain from the USB passband (audio 200 .. 5800 Hz within
 *            +-0.003 dB; audio <= -200 Hz and >= 6200 Hz at least 74 dB down); the frame is rint(y) saturated to int16.
 * One kernel, nothing else runs: no opt-in step is involved, the frames are ordinary frames and
 * ft8rx_enqueue_batch(h, ft8rx_staging_audio(h), n_out) is the intended next call.  Both entries first wait for the batches in flight.
 * Anything outside the definition is refused with -1 and an error text that names the argument. */
#define FT8RX_DDC_REAL_I16 0
#define FT8RX_DDC_REAL_F32 1
#define FT8RX_DDC_IQ_I16   2          /* I, Q interleaved */
#define FT8RX_DDC_IQ_F32   3
/* d_in: device, [n_streams][stream_stride] samples of `kind` (aligned to a sample).  d_audio: device, [n_out][180000]; NULL = the
 * handle's staging buffer.  d_audio_f32: optional device output [n_out][180000], y before rounding.  f_mixed_hz: optional host output
 * [n_out], the dial frequency actually mixed, w rate / 2^32 - 3000 (taken into [-rate/2, rate/2)).  n_out <= max_frames.  Asynchronous:
 * the kernel is queued on the handle's main stream, which every later call of the handle is ordered behind. */
int  ft8rx_ddc(ft8rx_handle* h, const void* d_in, int kind, int32_t rate_hz, int n_streams, uint64_t stream_stride,
               uint64_t n_samples, int n_out, const int32_t* src, const double* f_dial_hz, float gain,
               int16_t* d_audio, float* d_audio_f32, double* f_mixed_hz);
/* the same from host memory: staged through a handle-owned device buffer (allocated on first use, grown when a later call needs
 * more), result left in the staging audio buffer; returns when the frames are there */
int  ft8rx_ddc_host(ft8rx_handle* h, const void* in, int kind, int32_t rate_hz, int n_streams, uint64_t stream_stride,
                    uint64_t n_samples, int n_out, const int32_t* src, const double* f_dial_hz, float gain, double* f_mixed_hz);
/* host only, no GPU: the taps the kernels use.  stage 1 / 2 -> their count, and the first min(count, cap) of them in taps (float32;
 * taps may be NULL); 0 for a stage the rate does not have; -1 for a rate the build does not take (or another stage) */
int  ft8rx_ddc_taps(int32_t rate_hz, int stage, float* taps, int cap);
/* Streaming down-converter (extension): the definition above on a continuous stream, pushed in chunks of any
 * length, one stream set per handle.  Input index n and output index m = n / D are ABSOLUTE: they count from index 0 of the sample
 * clock and never restart; only n mod 2^32 enters the mixer phase, so it is exact at any n.  The stream begins at n_origin (a multiple
 * of 1008 D; live code passes 0) and is zero before it.  State, all on the handle, allocated by open, released by close or
 * ft8rx_destroy, nothing allocated in between: per stream a ring of the newest input samples in their own kind (a power of two that
 * holds one second and one tile's span), per channel a ring of the last 360000 outputs (two cycles; int16, optionally float32 before
 * rounding), a channel table of its own, 64-bit counters.  ft8rx_ddc / ft8rx_ddc_host between two pushes leave all of it untouched.
 * Outputs are produced in whole tiles of 1008 anchored at m = 1008 k, with the arithmetic of ft8rx_ddc's tile: every output is the same
 * bits however the stream was cut into chunks, and the first cycle of a stream with n_origin = 0 is ft8rx_ddc's output bit for bit.  An
 * output exists once its tile's last input has been pushed: at most 84 ms (one tile) + C2 R1 + C1 input samples (about 6 ms) after its
 * own sample.
 * open   kind, rate_hz, n_streams, n_out (<= max_frames), src, f_dial_hz, gain, f_mixed_hz: as ft8rx_ddc, refused by the same checks;
 *        keep_f32 != 0: also keep the float32 ring, y before rounding, 1.44 MB per channel (ft8rx_ddc_stream_frame_f32, read's y_f32);
 *        keep_f32 = FT8RX_DDC_KEEP_F32_FRAMES: the stream runs float frames -- the ring is kept and the
 *        spectrogram stage (ft8rx_ddc_stream_grid_*) reads it instead of the int16 ring.  Refused while a stream is open.
 * push   n_new samples of every stream, 1 .. rate_hz (one second): in = [n_streams][n_new] samples, host memory (copied through a
 *        page-locked buffer) or, on_device != 0, device memory; at most two copies per stream into the rings, then ONE kernel for every
 *        tile whose inputs are now complete.  Asynchronous on the handle's main stream.  m_produced: optional, the absolute index one
 *        past the last output produced so far.
 * frame  frame j position p = output m_first + p of channel j, for p < n_have; zero from n_have on, before the origin and from
 *        m_produced on.  m_first is a signed index passed as its 64-bit two's complement (it may be odd, negative, before the origin).
 *        d_audio: device [n_out][180000], NULL = the staging audio (ft8rx_enqueue_batch(h, ft8rx_staging_audio(h), n_out) is the
 *        intended next call).  Refused with -1 when part of the range has left the ring.  Waits for the batches in flight.
 * frame_f32  the same cut of the float32 ring into float32 frames, the same zero rules: d_audio device [n_out][180000] float, NULL =
 *        the float staging audio (ft8rx_enqueue_batch_f32(h, ft8rx_staging_audio_f32(h), n_out) is the intended next call).  Also
 *        refused, naming keep_f32, when the stream was opened without the float32 ring.
 * read  test aid: outputs [m_first, m_first + n) of every channel, all of them in the ring, -> host y_i16 / y_f32 [n_out][n] (either
 *        may be NULL); synchronous.
 * info   ring capacities in samples, samples pushed per stream, m_produced. */
int  ft8rx_ddc_stream_open(ft8rx_handle* h, int kind, int32_t rate_hz, int n_streams, int n_out, const int32_t* src,
                           const double* f_dial_hz, float gain, uint64_t n_origin, int keep_f32, double* f_mixed_hz);
int  ft8rx_ddc_stream_push(ft8rx_handle* h, const void* in, uint64_t n_new, int on_device, uint64_t* m_produced);
#define FT8RX_DDC_KEEP_F32_FRAMES 2
int  ft8rx_ddc_stream_frame(ft8rx_handle* h, uint64_t m_first, int n_have, int16_t* d_audio);
int  ft8rx_ddc_stream_frame_f32(ft8rx_handle* h, uint64_t m_first, int n_have, float* d_audio);
/* frames  (extension, opt-in; DESIGN.md section 19.7: live FT4, and the FT8 channels of a receiver that has both) frames of either length
 *        for chosen channels: frame i position p = output m_first + p of channel channels[i], for p < n_have; zero from n_have on,
 *        before the origin and from m_produced on -- the rules of frame.  frame_len: FT8RX_NSAMP (180000) or FT8RX_FT4_NSAMP (90000),
 *        anything else is refused by name; 0 <= n_have <= frame_len; 1 <= n_sel <= max_frames; every channels[i] in [0, n_out),
 *        repeats allowed; channels NULL = channels 0 .. n_sel - 1.  d_audio: device [n_sel][frame_len] int16; NULL = with frame_len
 *        90000 the handle's FT4 frame buffer (ft8rx_ft4_staging_audio; FT4's workspaces are allocated here if this is the handle's first
 *        FT4 call, all or nothing), with 180000 the staging audio.  ft8rx_ft4_enqueue_batch(h, ft8rx_ft4_staging_audio(h), n_sel), or
 *        ft8rx_enqueue_batch(h, ft8rx_staging_audio(h), n_sel), is the intended next call.  Refused with -1 when part of the range has
 *        left the ring.  Waits for the batches in flight.  The channel list lives in a table of the stream's (max_frames int32,
 *        allocated at the stream's first call here, released by close): it is uploaded, with one wait for the main stream, only when a
 *        call's list differs from the call before; nothing else is allocated or copied per call.  Serves the wide and the rational
 *        stream alike (their frames come from the same ring). */
int  ft8rx_ddc_stream_frames(ft8rx_handle* h, uint64_t m_first, int n_have, int frame_len, const int32_t* channels, int n_sel, int16_t* d_audio);
int  ft8rx_ddc_stream_read(ft8rx_handle* h, uint64_t m_first, int n, int16_t* y_i16, float* y_f32);
int  ft8rx_ddc_stream_info(ft8rx_handle* h, uint64_t* in_capacity, uint64_t* out_capacity, uint64_t* n_pushed, uint64_t* m_produced);
int  ft8rx_ddc_stream_close(ft8rx_handle* h);
/* Spectrogram stage behind the stream (extension, opt-in): the rows of ft8rx_spectrogram for every channel and
 * every hop, computed on the device straight from the output ring -- the waterfall and search grid of live wide input.  It serves a
 * plain stream and the stream behind a wide or rational one (ft8rx_ddc_wide_stream_*, ft8rx_ddc_rat_stream_*) alike.  With the grid
 * open at hop phase p0, row q of channel j is the Hann window, 3840-point real FFT and 10 log10(max(|X|^2, 1e-24)) (FT8RX_GRID_COLS
 * values) of the outputs y_j[p0 + 480 q - 3840, p0 + 480 q), zeros before the stream's first output; hop q is a row iff p0 + 480 q
 * lies beyond the first output's index, and it exists once m_produced >= p0 + 480 q.  A row depends on the ring's contents alone, so
 * it is the same bytes however the stream was cut into chunks, and it is byte for byte row h of ft8rx_spectrogram on the frame of
 * the outputs from m_first = p0 + 480 (q - h) on (8 <= h <= 375; 1 <= h <= 7 while only zeros lie before m_first).
 * grid_open  hop_phase in [0, 480), n_rows in [16, 750] (rows held per channel, the newest; 750 = two cycles): after any of the three
 *            stream opens and before the first push; refused otherwise and on a second open.  Allocates the grid ring
 *            [n_out][n_rows][FT8RX_GRID_COLS] float32; released by the stream's close or ft8rx_destroy.  Without it a push does
 *            nothing new.
 * push       (ft8rx_ddc_stream_push and the pre-stage pushes, unchanged) with the grid open also launches ONE kernel behind the
 *            tiles for the hops they complete (none, if they complete none; of more than n_rows new hops the newest n_rows).
 * grid_info  rows held [q_first_held, q_next), FT8RX_GRID_COLS, n_rows (any pointer may be NULL).
 * grid_read  rows [q_first, q_first + n) of every channel -> host rows [n_out][n][cols] float32, after the stream's work is done;
 *            refused with -1, naming the rows the ring holds, when one of them is not produced yet or no longer held. */
int  ft8rx_ddc_stream_grid_open(ft8rx_handle* h, int hop_phase, int n_rows);
int  ft8rx_ddc_stream_grid_info(ft8rx_handle* h, uint64_t* q_first_held, uint64_t* q_next, int32_t* cols, int32_t* n_rows);
int  ft8rx_ddc_stream_grid_read(ft8rx_handle* h, uint64_t q_first, int n, float* rows);
/* Wide pre-decimator (extension): ONE stream at rate_hz, a multiple of 48000 in [240000, 129600000] -- RTL-SDR
 * and HackRF (8-bit IQ), Airspy HF+ (IQ int16 at 384 / 768 kHz), direct-sampling receivers (real int16 at 64.8 / 129.6 MS/s) -- in front
 * of the down-converter above, which is used unchanged behind it.  rate_mid = the largest of 192000, 96000, 48000 that divides rate_hz
 * with R0 = rate_hz / rate_mid >= 2; R0 <= 1350 (ft8rx_ddc_wide_plan; anything else is refused, naming rate_hz).  Per channel j:
 *   mixer    w0 = round((f_dial + 3000) / rate 2^32) mod 2^32, f0 = w0 rate / 2^32 in [-rate/2, rate/2),
 *            u[n] = x[n] e^{-2 pi i (w0 n mod 2^32) / 2^32}: the wanted audio lands at the centre of the intermediate stream;
 *   filter   v[k] = g0 sum_j h0[j] u[k R0 + j - C0], h0 = the Kaiser recipe of section 16 at fs = rate_hz, pass 3200 Hz, stop
 *            rate_mid - 3200 Hz, 85 dB (ft8rx_ddc_wide_taps; 33 taps at 240 kHz, 145 at 2.4 MHz, 3883 at 64.8 MHz), g0 = 2 for the
 *            real kind and 1 for IQ;
 *   then     v, an IQ float32 stream at rate_mid, goes through the definition above (ft8rx_ddc / ft8rx_ddc_stream_*) with the dial
 *            f_dial - f0 (about -3000 Hz) and `gain`; f_mixed_hz = f0 + what that stage really mixed.
 * The passband and stopband promise of ft8rx_ddc holds for the whole chain (images of rate_mid at least 83 dB down).  Sample values:
 * the 16-bit kinds as they are; IQ uint8 x = 256 (u - 127.5), IQ int8 x = 256 s per component, so full scale and gain mean the same
 * for every kind.  Refusals return -1 with a text that names the argument. */
#define FT8RX_WIDE_REAL_I16 16
#define FT8RX_WIDE_IQ_I16   17         /* I, Q interleaved, as the two 8-bit kinds */
#define FT8RX_WIDE_IQ_U8    18
#define FT8RX_WIDE_IQ_I8    19
/* host only, no GPU: the plan of a rate -> 0 and rate_mid_hz / r0 (either may be NULL), or -1 for a rate that is refused */
int  ft8rx_ddc_wide_plan(int32_t rate_hz, int32_t* rate_mid_hz, int32_t* r0);
/* host only, no GPU: h0 of a rate -> its length and the first min(length, cap) taps (float32; taps may be NULL); -1 for a refused rate */
int  ft8rx_ddc_wide_taps(int32_t rate_hz, float* taps, int cap);
/* One call = one cycle: d_in = n_samples <= 15 rate_hz samples of `kind` on the device (aligned to a sample; zero before sample 0 and
 * after the last) -> n_out (<= max_frames) frames, channel j with the dial f_dial_hz[j] Hz from the stream's centre (the real kind: the
 * absolute frequency), in [-rate/2, rate/2).  The pre-stage writes [n_out][n_mid] intermediate samples into a handle-owned buffer
 * (allocated on first use, grown when a call needs more, as the tap tables of the channels), then ft8rx_ddc's kernel runs on it with
 * one stream per output.  d_audio, d_audio_f32, f_mixed_hz: as ft8rx_ddc.  Waits for the batches in flight and for the handle's main
 * stream (the tables are uploaded synchronously); the kernels are queued on that stream.  Refused while a wide stream is open. */
int  ft8rx_ddc_wide(ft8rx_handle* h, const void* d_in, int kind, int32_t rate_hz, uint64_t n_samples, int n_out,
                    const double* f_dial_hz, float gain, int16_t* d_audio, float* d_audio_f32, double* f_mixed_hz);
/* the same from host memory, staged through the handle's input buffer of ft8rx_ddc_host; result in the staging audio buffer; returns
 * when the frames are there */
int  ft8rx_ddc_wide_host(ft8rx_handle* h, const void* in, int kind, int32_t rate_hz, uint64_t n_samples, int n_out,
                         const double* f_dial_hz, float gain, double* f_mixed_hz);
/* The same on a continuous stream, one per handle.  Indices are absolute as in ft8rx_ddc_stream_*: input n, intermediate k = n / R0,
 * output m = n / (rate_hz / 12000); only n mod 2^32 enters the mixer phase (at 64.8 MS/s n passes 2^32 every 66 s).  State, allocated
 * by open and released by close or ft8rx_destroy, nothing in between: the last len(h0) - 1 + R0 input samples in their own kind, one
 * second of input (device and page-locked), one second of intermediate samples, the channels' tables, and the streaming
 * down-converter behind it (n_out IQ float32 streams at rate_mid), which open opens, push feeds on the device and close closes.
 * open      n_origin: absolute index of the first sample, a multiple of 1008 rate_hz / 12000; keep_f32 as ft8rx_ddc_stream_open.  Refused
 *           while a wide or a plain stream is open; while it is open ft8rx_ddc_stream_open / _push / _close and ft8rx_ddc_wide are refused.
 * push      n_new = 1 .. rate_hz samples, host memory or (on_device != 0) device memory: ONE kernel makes every intermediate sample
 *           whose last input has arrived (none, if the push completes none), at most two copies update the history, then the push
 *           of the stage behind.  Every sample is the same bits however the stream was cut into chunks, and with n_origin = 0 the
 *           first cycle is ft8rx_ddc_wide's bit for bit.  m_produced as ft8rx_ddc_stream_push.  Asynchronous on the main stream.
 * then      ft8rx_ddc_stream_frame / _read / _info work as on a plain stream (info counts intermediate samples).
 * read_mid  test aid: intermediate samples [k_first, k_first + n) of every channel -> host mid [n_out][n][2] float32 (re, im);
 *           held are the newest in_capacity (ft8rx_ddc_stream_info) samples; synchronous. */
int  ft8rx_ddc_wide_stream_open(ft8rx_handle* h, int kind, int32_t rate_hz, int n_out, const double* f_dial_hz, float gain,
                                uint64_t n_origin, int keep_f32, double* f_mixed_hz);
int  ft8rx_ddc_wide_stream_push(ft8rx_handle* h, const void* in, uint64_t n_new, int on_device, uint64_t* m_produced);
int  ft8rx_ddc_wide_stream_read_mid(ft8rx_handle* h, uint64_t k_first, int n, float* mid);
int  ft8rx_ddc_wide_stream_close(ft8rx_handle* h);
/* Rational resampler (extension): ONE stream at an integer rate_hz in [16000, 129600000] that neither ft8rx_ddc
 * nor ft8rx_ddc_wide takes -- sound cards at 44100 / 22050 / 16000 Hz, RTL-SDR at 2.048 / 1.024 MS/s and 250 kS/s, HackRF at 8 / 10 /
 * 20 MS/s -- in front of the down-converter above, which is used unchanged behind it.  Kinds: FT8RX_DDC_REAL_I16 .. FT8RX_DDC_IQ_F32 and
 * FT8RX_WIDE_IQ_U8 / FT8RX_WIDE_IQ_I8 (with the sample values of ft8rx_ddc_wide); any other is refused, naming kind.
 *   plan     for mid in 192000, 96000, 48000: g = gcd(rate, mid), L = mid / g, M = rate / g; rate_mid = the mid with the smallest L, ties
 *            to the largest; rate_mid = rate L / M.  The prototype h is the Kaiser recipe of section 16 at fs = rate L, pass 3200 Hz,
 *            stop min(rate, rate_mid) - 3200 Hz, 85 dB, odd length N, C = (N - 1) / 2, scaled to sum h = L (44100: 160 / 147, N = 1007;
 *            2048000: 3 / 32, N = 179; 10000000: 3 / 625, N = 3873).  Refused, naming rate_hz: L > 320 or N > 8448.
 *   mixer    w0 = round((f_dial + 3000) / rate 2^32) mod 2^32, u[n] = x[n] e^{-2 pi i (w0 n mod 2^32) / 2^32}, x = 0 outside the stream;
 *   filter   t_k = k M + C,  v[k] = g0 sum_{0 <= j < N, j = t_k (mod L)} h[j] u[(t_k - j) / L],  g0 = 2 for real kinds and 1 for IQ, all
 *            indices in 64-bit integers: intermediate sample k sits at input time k M / L, its last input is t_k / L;
 *   then     v, an IQ float32 stream at rate_mid, goes through ft8rx_ddc / ft8rx_ddc_stream_* with the dial f_dial - f0 and `gain`, as
 *            behind ft8rx_ddc_wide; f_mixed_hz = f0 + what that stage really mixed.
 * The passband and stopband promise of ft8rx_ddc holds for the whole chain.  Refusals return -1 with a text that names the argument. */
/* host only, no GPU: the plan of a rate -> 0 and rate_mid_hz / l / m / n_taps (each may be NULL), or -1 for a rate that is refused */
int  ft8rx_ddc_rat_plan(int32_t rate_hz, int32_t* rate_mid_hz, int32_t* l, int32_t* m, int32_t* n_taps);
/* host only, no GPU: h of a rate -> its length and the first min(length, cap) taps (float32; taps may be NULL); -1 for a refused rate */
int  ft8rx_ddc_rat_taps(int32_t rate_hz, float* taps, int cap);
/* One call = one cycle: n_samples <= 15 rate_hz samples of `kind` -> n_out frames.  Arguments, buffer ownership (the handle's buffers of
 * ft8rx_ddc_wide, grown when a call needs more) and ordering as ft8rx_ddc_wide / ft8rx_ddc_wide_host.  Refused while a rational or a wide
 * stream is open. */
int  ft8rx_ddc_rat(ft8rx_handle* h, const void* d_in, int kind, int32_t rate_hz, uint64_t n_samples, int n_out,
                   const double* f_dial_hz, float gain, int16_t* d_audio, float* d_audio_f32, double* f_mixed_hz);
int  ft8rx_ddc_rat_host(ft8rx_handle* h, const void* in, int kind, int32_t rate_hz, uint64_t n_samples, int n_out,
                        const double* f_dial_hz, float gain, double* f_mixed_hz);
/* The same on a continuous stream, one per handle, as ft8rx_ddc_wide_stream_*: indices are absolute (input n < 2^52, intermediate k);
 * state is allocated by open and released by close or ft8rx_destroy, nothing in between: the last ceil(N / L) input samples in their
 * own kind, one second of input (device and page-locked), one second of intermediate samples, the channels' tables, and the streaming
 * down-converter behind it.
 * open      n_origin: absolute index of the first sample; k_origin = n_origin L / M must be an integer and a multiple of
 *           1008 rate_mid / 12000 (0 always is; the grid is 18522 samples at 44100 Hz, 840000 at 10 MS/s); anything else is refused,
 *           naming n_origin.
 *           Refused while any stream is open; while it is open ft8rx_ddc_stream_open / _push / _close, ft8rx_ddc_wide_stream_open,
 *           ft8rx_ddc_wide and ft8rx_ddc_rat are refused (ft8rx_ddc is not, and leaves the stream alone).
 * push      n_new = 1 .. rate_hz samples, host or (on_device != 0) device memory: ONE kernel makes every intermediate sample whose last
 *           input has arrived (none, if the push completes none), at most two copies update the history, then the on-device push of
 *           the stage behind.  Every sample is the same bits however the stream was cut into chunks, and with n_origin = 0 the first
 *           cycle is ft8rx_ddc_rat's bit for bit.  Asynchronous on the main stream.
 * then      ft8rx_ddc_stream_frame / _read / _info work as on a plain stream (info counts intermediate samples).
 * read_mid  test aid, as ft8rx_ddc_wide_stream_read_mid. */
int  ft8rx_ddc_rat_stream_open(ft8rx_handle* h, int kind, int32_t rate_hz, int n_out, const double* f_dial_hz, float gain,
                               uint64_t n_origin, int keep_f32, double* f_mixed_hz);
int  ft8rx_ddc_rat_stream_push(ft8rx_handle* h, const void* in, uint64_t n_new, int on_device, uint64_t* m_produced);
int  ft8rx_ddc_rat_stream_read_mid(ft8rx_handle* h, uint64_t k_first, int n, float* mid);
int  ft8rx_ddc_rat_stream_close(ft8rx_handle* h);
/* Noise blanker (extension): impulse blanking of 12 kHz frames in place, an input stage like ft8rx_ddc and not a
 * handle setting -- the blanked frames are ordinary frames.  Everything is integer arithmetic that fits int32; pyft8_amd/blanker.py holds
 * the numpy twin, which gives the same bits.  A frame is 375 blocks of 480 samples, frames are independent.
 *   level   m_b = the element at sorted position 240 (from 0) of the 480 values |x| of block b (|-32768| = 32768);
 *           L_b = the element at sorted position 2 of the five values m[clamp(b + d, 0, 374)], d = -2 .. 2;
 *   hit     sample n of block b iff L_b > 0 and 256 |x[n]| > threshold_q8 L_b (L_b = 0, digital silence: the block passes untouched);
 *   gate    d[n] = distance to the nearest hit of the same frame; w = 0 for d <= guard, T[d - guard] for guard < d <= guard + taper,
 *           32768 beyond; T[j] = rint(32768 * 0.5 (1 - cos(pi j / (taper + 1)))), j = 1 .. taper (ft8rx_blank_taper);
 *   output  y[n] = (x[n] w[n] + 16384) >> 15 with an arithmetic shift: y = x where w = 32768, and a frame without hits keeps its bytes
 *           (it is not written at all);
 *   stats   per frame int32[4]: hits, samples with w < 32768, samples with w = 0, blocks with L_b = 0.
 * threshold_q8 = rint(256 k) in [512, 16384] (default k = 8: 5.4 sigma of Gaussian noise, whose median |x| is 0.6745 sigma), guard in
 * [0, 64] (default 6), taper in [0, 64] (default 6).  Anything else returns -1 with a text that names the argument. */
#define FT8RX_BLANK_THRESHOLD_Q8_DEFAULT 2048
#define FT8RX_BLANK_GUARD_DEFAULT        6
#define FT8RX_BLANK_TAPER_DEFAULT        6
#define FT8RX_BLANK_MIN_THRESHOLD_Q8     512
#define FT8RX_BLANK_MAX_THRESHOLD_Q8     16384
#define FT8RX_BLANK_MAX_GUARD            64
#define FT8RX_BLANK_MAX_TAPER            64
/* d_audio: device [n_frames][180000] int16 (aligned to a sample; 16-byte alignment takes the vector path), NULL = the staging audio;
 * n_frames in [1, max_frames].  stats: host [n_frames][4], optional; levels: host [n_frames][375][2] = (m_b, L_b), optional, a test
 * aid.  Waits for the batches in flight, then queues its kernels on the handle's main stream (the hit mask of every frame is complete
 * before the first sample is rewritten); returns after completion when stats or levels is given, otherwise at once. */
int  ft8rx_blank(ft8rx_handle* h, int16_t* d_audio, int n_frames, int32_t threshold_q8, int guard, int taper, int32_t* stats,
                 int32_t* levels);
/* the same from host memory: the frames are copied into the staging audio and blanked there; returns when they are
 * (ft8rx_enqueue_batch(h, ft8rx_staging_audio(h), n_frames) is the intended next call) */
int  ft8rx_blank_host(ft8rx_handle* h, const int16_t* audio, int n_frames, int32_t threshold_q8, int guard, int taper, int32_t* stats);
/* host only, no GPU: T[1 .. taper] -> taper, and the first min(taper, cap) entries in w (w may be NULL); -1 for taper outside [0, 64] */
int  ft8rx_blank_taper(int taper, int32_t* w, int cap);
/* Input-rate noise blanker (extension): the blanker above on the raw integer samples of ONE input stream at
 * their own rate, in front of ft8rx_ddc / ft8rx_ddc_wide / ft8rx_ddc_rat, whose device entries take the blanked samples.  A stand-alone
 * input stage: no down-converter kernel, ring or setting changes.  pyft8_amd/blank_in.py holds the numpy twin, which gives the same bits.
 *   kinds   FT8RX_DDC_REAL_I16, FT8RX_DDC_IQ_I16, FT8RX_WIDE_REAL_I16, FT8RX_WIDE_IQ_I16, FT8RX_WIDE_IQ_U8, FT8RX_WIDE_IQ_I8;
 *   value   per component c = x (int16), s (int8), 2 u - 255 (uint8); a[n] = |c| (real) or |cI| + |cQ| (IQ), at most 65536; a[n] = 0
 *           for every index outside the stream (before n_origin, behind the last sample of a one-shot call or a finished stream);
 *   level   block b is [b B, (b + 1) B) of the ABSOLUTE sample index; m_b = the element at sorted position B / 2 of its B values a;
 *           L_b = the element at sorted position 2 of m[b - 2 .. b + 2], no clamping (m = 0 outside the stream);
 *   hit     sample n of block b iff L_b > 0 and 256 a[n] > threshold_q8 L_b (2^24 and 2^30: int32);
 *   gate    as ft8rx_blank, d[n] = distance to the nearest hit of the stream, the same table ft8rx_blank_taper; per component
 *           c' = (c w + 16384) >> 15, stored as int16 / int8 c' or uint8 (c' + 255) >> 1; w = 32768 returns the input byte;
 *   stats   int64[4]: hits, samples with w < 32768, samples with w = 0, blocks [n_origin / B, n_end / B) with L_b = 0.
 * Streaming: after the inputs [.., n_end) exist the samples [n_origin, max(n_origin, (n_end / B - 2) B - (guard + taper))) are final
 * and released (ft8rx_blank_in_released) -- a function of n_end alone, so every released byte is the same however the stream was cut
 * into pushes; finish declares everything beyond n_end to be outside the stream and releases the rest.  A one-shot call on n samples
 * is the stream with n_origin = 0, pushed n samples and finished.  Latency: at most 3 B + guard + taper samples.
 * block: a power of two in [256, 4096]; threshold_q8 in [512, 16384]; guard, taper in [0, 64].  Anything else returns -1 with a text
 * that names the argument. */
#define FT8RX_BLANK_IN_BLOCK_DEFAULT             1024
#define FT8RX_BLANK_IN_MIN_BLOCK                 256
#define FT8RX_BLANK_IN_MAX_BLOCK                 4096
#define FT8RX_BLANK_IN_THRESHOLD_Q8_DEFAULT_REAL 2048    /* k = 8, as ft8rx_blank */
#define FT8RX_BLANK_IN_THRESHOLD_Q8_DEFAULT_IQ   1408    /* k = 5.5: the median of |I| + |Q| is 1.4866 sigma */
#define FT8RX_BLANK_IN_GUARD_DEFAULT             6
#define FT8RX_BLANK_IN_TAPER_DEFAULT             6
#define FT8RX_BLANK_IN_MAX_SAMPLES               2147483648ull   /* of a one-shot call */
#define FT8RX_BLANK_IN_MAX_PUSH                  268435456ull    /* of a stream's max_push */
/* d_samples: device, n_samples samples of `kind` (aligned to a sample; 16-byte alignment takes the vector path).  d_out: NULL = in
 * place, otherwise the samples are copied there first and blanked there (the same alignment rule).  stats: host [4], optional; levels:
 * host [ceil(n_samples / block)][2] = (m_b, L_b), optional, a test aid.  Waits for the batches in flight, then queues its work on the
 * handle's main stream; returns after completion when stats or levels is given, otherwise at once.  The workspaces (levels, hit mask,
 * partial counters) belong to the handle: made at the first call, grown when a call needs more. */
int  ft8rx_blank_in(ft8rx_handle* h, void* d_samples, int kind, uint64_t n_samples, int block, int32_t threshold_q8, int guard, int taper,
                    void* d_out, int64_t* stats, int32_t* levels);
/* the same from host memory: copied into a device buffer of the handle (made at the first call, grown on demand) and blanked there;
 * *d_out = that buffer, valid until the next ft8rx_blank_in / ft8rx_blank_in_host call.  Returns when the samples have been copied
 * (and blanked, when stats is given); what is queued on the main stream next -- the d_in entry of a down-converter -- follows it. */
int  ft8rx_blank_in_host(ft8rx_handle* h, const void* samples, int kind, uint64_t n_samples, int block, int32_t threshold_q8, int guard, int taper,
                         int64_t* stats, void** d_out);
/* The stream: one per handle, independent of any down-converter stream (ft8rx_ddc* calls in between leave it alone).  open allocates
 * everything (two work buffers of 4 block + guard + taper + max_push samples, the rings, a page-locked chunk), close or ft8rx_destroy
 * releases it, nothing is allocated in between.  n_origin: the absolute index of the first sample, at most 2^53. */
int  ft8rx_blank_in_stream_open(ft8rx_handle* h, int kind, int block, int32_t threshold_q8, int guard, int taper, uint64_t n_origin,
                                uint64_t max_push);
/* n_new in [0, max_push] samples from host memory or (on_device) device memory; finish != 0: the stream ends behind them, and only
 * info and close are accepted afterwards.  -> *d_out = the device address of the newly released samples, *n_first their absolute
 * index, *n_out their count (0 is possible, and up to block more than n_new; finish: everything left); each may be NULL.  The samples
 * stay valid until the next push.  Queued on the handle's main stream; does not wait for it. */
int  ft8rx_blank_in_stream_push(ft8rx_handle* h, const void* in, uint64_t n_new, int on_device, int finish, void** d_out, uint64_t* n_first,
                                uint64_t* n_out);
/* samples pushed, samples released (absolute index of the first one that is not), the cumulative stats [4]; each may be NULL.  Waits
 * for the main stream when stats is given. */
int  ft8rx_blank_in_stream_info(ft8rx_handle* h, uint64_t* n_pushed, uint64_t* n_released, int64_t* stats);
int  ft8rx_blank_in_stream_close(ft8rx_handle* h);
/* host only, no GPU: *released = the absolute index of the first sample that is not final once [.., n_end) exist -> 0, or -1 for
 * arguments outside the definition (n_end < n_origin included) */
int  ft8rx_blank_in_released(uint64_t n_origin, uint64_t n_end, int block, int guard, int taper, uint64_t* released);
/* Panorama (extension): the averaged power spectrum of ONE raw input stream of any kind (FT8RX_DDC_*,
 * FT8RX_WIDE_*) at its own rate, and how often it touched the converter's rails.  A stand-alone input stage: nothing else changes, and
 * it runs beside any down-converter or input blanker stream.  pyft8_amd/pan.py holds the float64 twin.
 *   value   the sample on the int16 scale (uint8 256 (u - 127.5), int8 256 s, the others as they are); a real kind has Im = 0;
 *   window  w = the ABSOLUTE samples [w N, (w + 1) N), N = n_fft, weighted by the periodic Hann window ft8rx_pan_window; only
 *           complete windows count; X_w = the N-point DFT in float32, p_w[k] = Re^2 + Im^2;
 *   row     r = the windows [r A, (r + 1) A), A = n_avg: P_r[j] = the float32 SUM of p_w[k(j)] in window order, not normalised; only
 *           rows whose samples all lie in the stream exist, the first being ceil(ceil(n_origin / N) / A);
 *   bins    IQ kinds N per row, ascending frequency: j is bin k = (j + N / 2) mod N at (j - N / 2) rate / N; real kinds N / 2, j = k;
 *   stats   int32 [2] per row, exact: samples with a component at the format's lowest or highest code (int16 -32768 / 32767, int8
 *           -128 / 127, uint8 0 / 255), and the largest |c| of a component, c = x (int16), s (int8), 2 u - 255 (uint8); float kinds 0, 0.
 * n_fft: a power of two in [256, 8192]; n_avg in [1, 65536].  Anything else returns -1 with a text that names the argument. */
#define FT8RX_PAN_FFT_DEFAULT  2048
#define FT8RX_PAN_MIN_FFT      256
#define FT8RX_PAN_MAX_FFT      8192
#define FT8RX_PAN_MAX_AVG      65536
#define FT8RX_PAN_ROWS_DEFAULT 256
#define FT8RX_PAN_MAX_ROWS     65536
#define FT8RX_PAN_MAX_SAMPLES  2147483648ull   /* of a one-shot call */
#define FT8RX_PAN_MAX_PUSH     268435456ull    /* of a stream's max_push */
/* host only, no GPU: the weights, computed in double and rounded once -> n_fft, and the first min(n_fft, cap) of them in w (w may be
 * NULL); -1 for an n_fft outside the definition */
int  ft8rx_pan_window(int n_fft, float* w, int cap);
/* host only, no GPU: rows[0] = the first row of a stream that began at n_origin, rows[1] = the first row that is NOT complete once
 * the samples [n_origin, n_end) exist (rows[1] - rows[0] rows exist) -> 0, or -1 for arguments outside the definition */
int  ft8rx_pan_rows_done(uint64_t n_origin, uint64_t n_end, int n_fft, int n_avg, uint64_t* rows);
/* The one-shot on n_samples device samples of `kind` from index 0 (aligned to a component; samples behind the last complete row are
 * not read): *n_rows_out = (n_samples / n_fft) / n_avg rows -> rows, host [n_rows][bins], and stats, host [n_rows][2]; each may be
 * NULL.  Waits for the batches in flight, queues its work on the handle's main stream and returns after completion.  The workspaces
 * belong to the handle: made at the first call, grown when a call needs more. */
int  ft8rx_pan(ft8rx_handle* h, const void* d_samples, int kind, uint64_t n_samples, int n_fft, int n_avg, float* rows, int32_t* stats,
               uint64_t* n_rows_out);
/* the same from host memory: the samples are copied into a device buffer of the handle first */
int  ft8rx_pan_host(ft8rx_handle* h, const void* samples, int kind, uint64_t n_samples, int n_fft, int n_avg, float* rows, int32_t* stats,
                    uint64_t* n_rows_out);
/* The stream: one per handle, independent of every other stream of the handle.  open allocates everything (a work buffer of
 * n_fft - 1 + max_push samples, a leftover of n_fft, a page-locked chunk, one tile of window powers, the ring of n_rows + 1 rows),
 * close or ft8rx_destroy releases it, nothing is allocated in between.  n_rows in [1, 65536]: the finished rows the ring keeps;
 * n_origin: the absolute index of the first sample, at most 2^53. */
int  ft8rx_pan_stream_open(ft8rx_handle* h, int kind, int n_fft, int n_avg, int n_rows, uint64_t n_origin, uint64_t max_push);
/* n_new in [0, max_push] samples from host memory or (on_device) device memory, copied once into the work buffer: *d_samples = the
 * device address of the chunk's first sample there, valid until the next push -- what a down-converter's device push takes, so that a
 * chunk crosses the bus once; *rows_done = the first row that is not complete yet.  Each may be NULL.  Queued on the handle's main
 * stream; does not wait for it. */
int  ft8rx_pan_stream_push(ft8rx_handle* h, const void* in, uint64_t n_new, int on_device, void** d_samples, uint64_t* rows_done);
/* the finished rows [r_first, r_first + n) -> rows, host [n][bins], and stats, host [n][2] (each may be NULL); rows that are not
 * complete yet or that the ring no longer holds are refused, naming the rows it holds.  Returns after completion. */
int  ft8rx_pan_stream_read(ft8rx_handle* h, uint64_t r_first, int n, float* rows, int32_t* stats);
/* samples pushed, the first row that is not complete, the oldest row the ring holds, bins per row; each may be NULL */
int  ft8rx_pan_stream_info(ft8rx_handle* h, uint64_t* n_pushed, uint64_t* rows_done, uint64_t* r_lo, int* bins);
int  ft8rx_pan_stream_close(ft8rx_handle* h);
/* Local re-search of the reference's subtraction experiment (tests/pipeline/receiver_sub.py:434-445: after a signal has been
 * subtracted, search(f0_idx - 2 .. f0_idx + 1, ignore_sync_score_min = True)): mask[n_frames][cfg.f0_hi - cfg.f0_lo], one byte per
 * search column.  While a mask is set, the candidate selection of every batch (Receiver.search, receiver.py:338-367) takes ONLY the
 * columns whose byte is non-zero and every score above 0 instead of above sync_score_min; order (score descending, stable) and the
 * max_cands cap as always.  mask = NULL: back to the configured search.  Batches in flight finish under the setting they started with. */
int  ft8rx_set_search_mask(ft8rx_handle* h, const uint8_t* mask, int n_frames);
int  ft8rx_set_profiling(ft8rx_handle* h, int on);
int  ft8rx_get_stage_times(ft8rx_handle* h, int* n, const char** names, float* ms);

/* ---- stage entry points (parity tests; each mirrors one reference function) ---------------- */
/* AudioIn.get_hop_spectrum x375 (receiver.py:288-293): grid [n][376][FT8RX_GRID_COLS] */
int  ft8rx_spectrogram(ft8rx_handle* h, const int16_t* audio, int n_frames, float* grid);
/* the same of float32 frames: the samples as they are, zeros before the frame start */
int  ft8rx_spectrogram_f32(ft8rx_handle* h, const float* audio, int n_frames, float* grid);
/* streaming mode: ONE call of AudioIn.get_hop_spectrum (receiver.py:288-293): the last 3840 int16 samples -> FT8RX_GRID_COLS dB values */
int  ft8rx_hop_spectrum(ft8rx_handle* h, const int16_t* window3840, float* row);
/* Receiver.search (receiver.py:338-367): per frame <= max_cands (f0,h0,score), sorted */
int  ft8rx_sync_search(ft8rx_handle* h, const float* grid, int n_frames,
                       int32_t* f0_idx, int32_t* h0_idx, float* score, int32_t* counts);
/* The inner loops of Receiver.search (receiver.py:341-349) for ANY f0 index range [f0_lo, f0_hi) the grid can hold (4 <= f0_lo,
 * f0_hi <= FT8RX_GRID_COLS - 15), whatever range the handle was created for: per frame and f0 the first strict maximum of the Costas
 * score over the handle's h0 range, starting from 0 -- score [n][f0_hi - f0_lo] and its h0 (0 / 0 where no score is positive).  The
 * threshold, stable sort and cut (receiver.py:350-367) are the caller's; Receiver.search uses this for `search_f_idxs` lists that
 * are not the configured range. */
int  ft8rx_sync_scores(ft8rx_handle* h, const float* grid, int n_frames, int f0_lo, int f0_hi, float* score, int32_t* h0_idx);
/* ft8rx_sync_scores with weak mode's three-block score (k_sync3; ft8rx_set_weak), whatever the handle's setting */
int  ft8rx_sync_scores_weak(ft8rx_handle* h, const float* grid, int n_frames, int f0_lo, int f0_hi, float* score, int32_t* h0_idx);
/* Candidate._get_llr_grid/_dB_to_llr (receiver.py:136-138, 208-222) for n (frame,f0,h0) triples */
int  ft8rx_llr_grid(ft8rx_handle* h, const float* grid, int n_frames, int n, const int32_t* frame,
                    const int32_t* f0_idx, const int32_t* h0_idx, float* llr /*[n][174]*/, float* sd, int32_t* snr);
/* AudioIn.get_cycle_spectrum (receiver.py:280-286): spec [n][FT8RX_SPEC_BINS] complex64 */
int  ft8rx_cycle_spectrum(ft8rx_handle* h, const int16_t* audio, int n_frames, float* spec);
/* the same of float32 frames */
int  ft8rx_cycle_spectrum_f32(ft8rx_handle* h, const float* audio, int n_frames, float* spec);
/* Candidate._get_llr_fine (receiver.py:140-206) for n (frame,f0,h0) triples; sgrid [n][79][8] may be NULL.
 * ret[i]: 1 continue, 0 Costas gate failed, -1 sd gate failed */
int  ft8rx_fine(ft8rx_handle* h, const float* spec, int n_frames, int n, const int32_t* frame,
                const int32_t* f0_idx, const int32_t* h0_idx, int32_t* ret, int32_t* ttweak, int32_t* ftweak,
                int32_t* nsync, float* llr, float* sd, int32_t* snr, float* sgrid);
/* ft8rx_fine with weak mode's joint scan (k_fine_weak; ft8rx_set_weak), whatever the handle's setting: ret[i] is 1 or 0 (no sd
 * gate), sd / snr are reported all the same.  Triples must lie in [0, n_frames) x [4, FT8RX_MAX_F0) x [FT8RX_MIN_H0, FT8RX_MAX_H0). */
int  ft8rx_fine_weak(ft8rx_handle* h, const float* spec, int n_frames, int n, const int32_t* frame,
                     const int32_t* f0_idx, const int32_t* h0_idx, int32_t* ret, int32_t* ttweak, int32_t* ftweak,
                     int32_t* nsync, float* llr, float* sd, int32_t* snr, float* sgrid);
/* ldpc_decode(llr, max_ncheck0, max_iters) (decoders.py:153-171) on n vectors.
 * ok[i]=1 => msg; has_out[i]=1 => llr_out[i] holds the mutated llr (the reference's third return) */
int  ft8rx_ldpc(ft8rx_handle* h, const float* llr, int n, int max_ncheck0, int max_iters,
                int32_t* ok, uint64_t* msg_lo, uint64_t* msg_hi, int32_t* n_its, int32_t* has_out, float* llr_out);
/* osd_012(llr, singleflips, doubleflips) (decoders.py:223-272) on n vectors; 0 <= singleflips, doubleflips <= 91 (all basis positions) */
int  ft8rx_osd(ft8rx_handle* h, const float* llr, int n, int singleflips, int doubleflips,
               int32_t* ok, uint64_t* msg_lo, uint64_t* msg_hi, int32_t* trial);
/* same with the build's extension knobs: tripleflips = order-3 depth, max_hd = acceptance gate (0 = off); hd[i] (optional) = the
 * Hamming distance of the accepted codeword to the hard decisions */
int  ft8rx_osd_ext(ft8rx_handle* h, const float* llr, int n, int singleflips, int doubleflips, int tripleflips, int max_hd,
                   int32_t* ok, uint64_t* msg_lo, uint64_t* msg_hi, int32_t* trial, int32_t* hd);
/* crc_unpack91 (decoders.py:117-131) on n x 91 soft/hard values: res 0 = no CRC, 1 = CRC ok but unpack None, 2 = tuple */
int  ft8rx_crc_valid(ft8rx_handle* h, const float* cw91, int n, int32_t* res, uint64_t* msg_lo, uint64_t* msg_hi);
/* unpack() validity predicate (decoders.py:16-115) on n 77-bit words */
int  ft8rx_valid77(ft8rx_handle* h, const uint64_t* msg_lo, const uint64_t* msg_hi, int n, int32_t* valid);
/* the same predicate with opt-in message types (FT8RX_MT_* bits; mask = 0 is ft8rx_valid77), as the GOOD91 and BP steps
 * apply it -- an OSD trial additionally never accepts free text or telemetry */
int  ft8rx_valid77_ext(ft8rx_handle* h, const uint64_t* msg_lo, const uint64_t* msg_hi, int n, int32_t mask, int32_t* valid);
/* Workload generator (modelled on transmitter.py:41-70): n_frames synthetic 15-s frames of
 * n_signals GFSK signals + Philox white noise, written to the device buffer d_audio[n_frames][180000] int16.
 * signal_table: n_frames*n_signals records laid out as pyft8_amd/synth.py:SIGNAL_DTYPE; pulse_cumsum: 5761 doubles. */
int  ft8rx_synth_frames(ft8rx_handle* h, uint64_t seed, int first_index, int n_frames, int n_signals,
                        const void* signal_table, int signal_bytes, const double* pulse_cumsum, int16_t* d_audio);
/* same; no_noise != 0 leaves the Philox noise out (parity tests of the signal part against the numpy twin pyft8_amd/synth.py) */
int  ft8rx_synth_frames_ex(ft8rx_handle* h, uint64_t seed, int first_index, int n_frames, int n_signals,
                           const void* signal_table, int signal_bytes, const double* pulse_cumsum, int16_t* d_audio, int no_noise);
/* Host message layer (pure host code, no GPU needed): replays each frame's records + events in the reference's emit
 * order -- hash-table side effects of every unpack() call (decoders.py:44,92; databases.py:10-26), duplicate filter
 * (receiver.py:51-66), round/llr_sd ordering of manage_cycle (receiver.py:389-398) -- and renders the message tuples.
 * records [n_frames][max_cands], events [n_frames][FT8RX_EVENT_CAP]; out [n_frames][max_msgs]; out_counts[f] <= max_msgs.
 *   table == NULL : every frame gets a fresh call-hash table (independent batched frames, the parity semantics of
 *                   DESIGN.md section 1); frames are spread over n_threads host threads.
 *   table != NULL : frames are replayed in order on the caller's thread against that persistent table, which they update --
 *                   the reference's process-global `call_hashes` (databases.py:8): a hashed / non-standard call heard in
 *                   cycle N resolves `<...>` in cycle N+1.  This is what the streaming receiver uses.
 * flags (optional, [n_frames]): FT8RX_PKG_* bits per frame.
 * The packager runs its frames on a persistent pool of worker threads owned by the library; ONE ft8rx_package_batch /
 * ft8rx_package_packed call uses the pool at a time, concurrent callers of a process queue behind each other. */
#define FT8RX_PKG_MSG_TRUNCATED    1   /* more than max_msgs messages: the list was cut (size max_msgs >= cfg.max_cands to rule it out) */
#define FT8RX_PKG_EVENTS_TRUNCATED 2   /* event_counts[f] > FT8RX_EVENT_CAP: unpack() calls were dropped, `<...>` strings may differ */
int  ft8rx_package_batch(const ft8rx_record* records, const int32_t* counts, const ft8rx_event* events, const int32_t* event_counts,
                         int n_frames, int max_cands, ft8rx_message* out, int max_msgs, int32_t* out_counts, int n_threads,
                         ft8rx_hashes* table, int32_t* flags);
/* ft8rx_package_batch for records of a handle with msg_types = mask: the words of the opt-in types are rendered too (their
 * standard calls enter the call-hash table, hash fields are looked up in it), into the wider ft8rx_message_ext.  mask = 0 renders
 * exactly what ft8rx_package_batch does.  The packed path (ft8rx_package_packed) has no _ext form. */
int  ft8rx_package_batch_ext(const ft8rx_record* records, const int32_t* counts, const ft8rx_event* events, const int32_t* event_counts,
                             int n_frames, int max_cands, ft8rx_message_ext* out, int max_msgs, int32_t* out_counts, int n_threads,
                             ft8rx_hashes* table, int32_t* flags, int32_t mask);
/* Multi-pass decoding (extension; no GPU needed): append to each frame's message list out[f][0..out_counts[f])
 * those messages of a later pass, add[f][0..add_counts[f]), whose text the frame does not have yet (pad[0] = pass_tag marks them);
 * the same messages, untagged, go to fresh[f] (optional; [n_frames][max_add]) -- the input of the next subtraction sweep.
 * drop_osd != 0 ignores the later pass's OSD decodes (first CRC-valid trial wins there: the source of false decodes). */
int  ft8rx_merge_messages(ft8rx_message* out, int32_t* out_counts, int max_out, const ft8rx_message* add, const int32_t* add_counts,
                          int max_add, int n_frames, int pass_tag, int drop_osd, ft8rx_message* fresh, int32_t* fresh_counts);
/* The whole drop-in in one call -- what a compiled-language binding (cgo / JNI / N-API) would bind: host audio [n_frames][180000]
 * int16 in, the frames' messages out (Receiver's on_message payloads before string formatting, in the reference's emit order):
 * ft8rx_decode_batch followed by ft8rx_package_batch on the handle's own result buffers.  out: [n_frames][max_msgs] (max_msgs >=
 * cfg.max_cands rules truncation out); n_threads / table / flags as for ft8rx_package_batch. */
int  ft8rx_decode_messages(ft8rx_handle* h, const int16_t* audio, int n_frames, ft8rx_message* out, int max_msgs, int32_t* out_counts,
                           int n_threads, ft8rx_hashes* table, int32_t* flags);
/* the same from float32 frames: ft8rx_decode_batch_f32 followed by ft8rx_package_batch */
int  ft8rx_decode_messages_f32(ft8rx_handle* h, const float* audio, int n_frames, ft8rx_message* out, int max_msgs, int32_t* out_counts,
                               int n_threads, ft8rx_hashes* table, int32_t* flags);
/* the persistent call-hash table (databases.py:8-26 `call_hashes` + add_call_hashes) */
ft8rx_hashes* ft8rx_hashes_create(void);
void ft8rx_hashes_destroy(ft8rx_hashes* t);
int  ft8rx_hashes_clear(ft8rx_hashes* t);
int  ft8rx_hashes_add(ft8rx_hashes* t, const char* call);           /* add_call_hashes(call) */
int  ft8rx_hashes_size(const ft8rx_hashes* t);                       /* number of (hash, nbits) keys */
/* Optional reject log: with a path set, every callsign that fails the plausibility test is appended to that file, one per line,
 * as the reference does unconditionally to ./rejected_callsigns.txt (decoders.py:114-115).  NULL or "" turns it off (default). */
int  ft8rx_set_reject_log(const char* path);
/* the handle's own device audio buffer ([max_frames][180000] int16) and a D2H copy helper (tests, tools) */
int16_t* ft8rx_staging_audio(ft8rx_handle* h);
/* ... and the one of float32 frames ([max_frames][180000] float), allocated on first use */
float* ft8rx_staging_audio_f32(ft8rx_handle* h);
int  ft8rx_copy_to_host(ft8rx_handle* h, void* dst, const void* d_src, uint64_t bytes);
/* Asynchronous device -> page-locked-host copies on the handle's result-copy stream (the one stream no decode kernel waits behind; a
 * copy on any other stream of the process shares a hardware queue with a decode stream and holds its kernels back while it runs).
 * For consumers of device-side results -- the gather on rank `dst` (pyft8_amd/distributed.py).  32 tickets: the 33rd call waits for the oldest.
 *   ft8rx_d2h_async: enqueue; *ticket identifies the copy     ft8rx_d2h_query: 1 landed, 0 not yet, < 0 error
 *   ft8rx_d2h_event: the hipEvent_t recorded behind the copy (valid until 32 more copies were issued), e.g. for ft8rx_packed_output_fence */
int   ft8rx_d2h_async(ft8rx_handle* h, void* dst, const void* d_src, uint64_t bytes, int32_t* ticket);
int   ft8rx_d2h_query(ft8rx_handle* h, int32_t ticket);
void* ft8rx_d2h_event(ft8rx_handle* h, int32_t ticket);
/* ---- signal subtraction ------------------------------------------------------
 * One decoded signal to remove: its 79 tones (Costas + Gray-coded codeword), refined frequency and start time.  96 bytes. */
typedef struct {
    double  fHz, tsec;               /* candidate origin after fine sync (receiver.py:166) */
    uint8_t tones[79];
    uint8_t pad;
} ft8rx_subsig;
/* Stands in for Receiver.subtract_signal of the reference's subtraction experiment (tests/pipeline/receiver_sub.py:380-402,
 * with PyFT8/transmitter.py:41-70 for the GFSK model): for every frame, signals sigs[frame][0 .. counts[frame]) are subtracted in
 * list order from a float32 working copy of the device-resident int16 audio; the residual is rounded back to int16 in place
 * (d_audio is a device pointer).  audio_f32_out (host, optional, [n_frames][180000]) receives the float32 residual. */
int  ft8rx_subtract(ft8rx_handle* h, int16_t* d_audio, int n_frames, ft8rx_subsig* sigs, const int32_t* counts,
                    int max_sigs, int refine, float* audio_f32_out);
/* the same on device-resident float32 frames: the working copy is filled from d_audio without conversion and
 * written back without rounding; everything between is ft8rx_subtract's, refine included */
int  ft8rx_subtract_f32(ft8rx_handle* h, float* d_audio, int n_frames, ft8rx_subsig* sigs, const int32_t* counts,
                        int max_sigs, int refine, float* audio_f32_out);
/* refine = 0: the given (fHz, tsec) are used as they are (the reference's arithmetic).  refine = 1 (extension): before a signal is
 * subtracted its origin is re-estimated with the same signal model over all 79 symbols -- start sample within [-150, +20] ms and
 * frequency within [-1.75, +5.75] Hz of the given values -- and `sigs` is updated with the refined origins.  (The decoder's
 * tsec/fHz follow the search grid's conventions and sit ~75 ms / ~1.9 Hz off the true start; cancellation needs a few ms.)
 * refine = 2 (extension): the same re-estimation on a copy of the residual that is mixed down to the signal's centre frequency and
 * decimated by 32 (time grid 2.67 ms): same accuracy and decode yield, a third of the time; the subtraction itself stays at full
 * rate with the exact model.  This is what Receiver's multi-pass decode uses.
 * refine = 3: Candidate.refine_time_origin of the reference's experiment (receiver_sub.py:58-72) -- before each signal is subtracted
 * its start time is re-estimated in 12 steps of 5 ms from tb_0 - 6 on the spectrum of the residual so far (untapered 1000-bin slice,
 * score = max over the three Costas blocks), tsec = tb / 200, fHz = int(0.5 + 16 fHz) / 16 -- then subtract_signal as with refine = 0.
 * `sigs` returns the re-estimated origins. */
/* Multi-pass decoding: the signals a subtraction sweep removes = every message of a frame with snr > min_snr, in emit order, with the
 * tones of its codeword (ft8rx_encode_tones of the candidate's word) and the origin its message dict reports (receiver.py:166).
 * sigs: [n_frames][max_sigs]; returns the largest per-frame count (or < 0). */
int  ft8rx_subtraction_list(const ft8rx_message* msgs, const int32_t* counts, int max_msgs, const ft8rx_record* records, int max_cands,
                            int n_frames, int min_snr, ft8rx_subsig* sigs, int max_sigs, int32_t* sig_counts);
/* 77-bit words -> the 79 transmitted tones (CRC-14, LDPC(174,91) encode, Gray map, Costas framing; reference
 * transmitter.py:181-223 `encode_bits77`).  Host function, no GPU.  tones: [n][79]. */
int  ft8rx_encode_tones(const uint64_t* msg_lo, const uint64_t* msg_hi, int n, uint8_t* tones);
/* Page-locked host memory for audio handed to ft8rx_decode_batch: copies from it are true asynchronous DMA that overlaps the
 * kernels of earlier chunks (pageable memory works too, at a lower PCIe-inclusive rate).  Free with ft8rx_free_host. */
void* ft8rx_alloc_host(ft8rx_handle* h, uint64_t bytes);
int  ft8rx_free_host(ft8rx_handle* h, void* p);               /* h may be NULL */
/* arithmetic-contract probes: which 0 = log10f, 1 = tanhf; 2 = forward FFT of length n (x = interleaved complex) */
int  ft8rx_math_probe(ft8rx_handle* h, int which, const float* x, int n, float* y);

/* ---- FT4 (extension) ------------------------------------------------------
 * Opt-in decoding of 7.5-s FT4 frames: int16 mono at 12 kHz, 90000 samples, nominal signal start 0.5 s into the slot.  FT4 shares
 * FT8's 77-bit messages, CRC-14 and LDPC(174,91); the front end is its own (kernels/ft4.hpp; pyft8_amd/ft4.py is the float64 twin
 * that defines it): a 618 x 577 dB grid (1152-point FFT every 144 samples: two bins per tone, four rows per symbol), a search over
 * the four Costas blocks, per candidate a 9 x 5 fine sync on the audio (steps of 36 samples and 2.6042 Hz) and a symbol-synchronous
 * demodulator; behind it BP(bp_nc0_b, bp_iters_b), then OSD(osd_single, osd_double) under a Hamming-distance gate, with the 77 bits
 * descrambled between the CRC test and the validity predicate.  The layout does not depend on FT8RX_WIDE; the search range is
 * 12.5 .. 5900 Hz and -0.5 .. +2.0 s unless ft8rx_ft4_set_range narrows it; max_cands is the handle's.
 * Records: f0_idx = bin (10.41667 Hz), h0_idx = row (12 ms), ttweak = dt / 36 samples, ftweak = df / 2.60417 Hz, so that
 *   t = (144 h0_idx + 36 ttweak) / 12000 s,  f = 10.41667 f0_idx + 2.60417 ftweak Hz (tone 0);
 * snr_fine = the demodulator's report, score = the search score (grid_sd = fine_sd = score), ipass 4 / method FT8RX_M_LDPC_B for a BP
 * decode, ipass 5 / FT8RX_M_OSD with osd_hd for an OSD decode; msg_lo / msg_hi hold the descrambled word.  Every decode logs one
 * event.  Results are fetched and packaged through the FT8 calls (ft8rx_fetch_results, ft8rx_package_batch / _ext).
 * The workspaces (1.6 MB per frame of max_frames, 2.1 KB per candidate slot) are allocated at the first FT4 call on a
 * handle, all or nothing; a handle that never decodes FT4 allocates and launches nothing of this.
 * FT4 runs with msg_types; it is refused, by name, while ft8rx_set_ap_calls, ft8rx_set_recall, ft8rx_set_weak, ft8rx_set_reports or
 * the packed output is active.  No foreign FT4 signal has been decoded yet: the mode is pinned to the protocol constants and the twin. */
#define FT8RX_FT4_NSAMP 90000
#define FT8RX_FT4_ROWS  618
#define FT8RX_FT4_COLS  577
#define FT8RX_FT4_SYNC_MIN_DEFAULT   100.0f
#define FT8RX_FT4_WEAK_MIN_DEFAULT   16.17f  /* the weak search's threshold: as many noise candidates as sync_min = 100 (section 19.10) */
#define FT8RX_FT4_OSD_MAX_HD_DEFAULT 40      /* the largest gate without a false decode on 2048 noise frames (profiles/ft4_notes.md) */
/* host int16 [n_frames][90000] -> records [n_frames][max_cands], counts, events [n_frames][FT8RX_EVENT_CAP], event_counts */
int  ft8rx_ft4_decode_batch(ft8rx_handle* h, const int16_t* audio, int n_frames, ft8rx_record* records, int32_t* counts,
                            ft8rx_event* events, int32_t* event_counts);
/* the same on device-resident frames (4-byte aligned); the results are fetched with ft8rx_fetch_results */
int  ft8rx_ft4_enqueue_batch(ft8rx_handle* h, const int16_t* d_audio, int n_frames);
/* the knobs: the search threshold and OSD's distance gate; 0 = the default */
int  ft8rx_ft4_set(ft8rx_handle* h, float sync_min, int32_t osd_max_hd);
/* the search range in bins [f0_lo, f0_hi) within [0, 571) and rows [h0_lo, h0_hi) within [-1024, 1024); all four 0 = the default */
int  ft8rx_ft4_set_range(ft8rx_handle* h, int32_t f0_lo, int32_t f0_hi, int32_t h0_lo, int32_t h0_hi);
/* bytes of FT4 workspace the handle holds (0 until its first FT4 call) and the current knobs and range [4]; any pointer may be NULL */
int  ft8rx_ft4_info(ft8rx_handle* h, uint64_t* workspace_bytes, float* sync_min, int32_t* osd_max_hd, int32_t* range);
/* ft8rx_ft4_decode_batch followed by ft8rx_package_batch (msg_types = 0) -- with msg_types set, use ft8rx_ft4_decode_batch and
 * ft8rx_package_batch_ext */
int  ft8rx_ft4_decode_messages(ft8rx_handle* h, const int16_t* audio, int n_frames, ft8rx_message* out, int max_msgs, int32_t* out_counts,
                               int n_threads, ft8rx_hashes* table, int32_t* flags);
/* stage entry points (tests).  grid: dB [n_frames][618][577]; power (optional): the same layout before the logarithm */
int  ft8rx_ft4_grid(ft8rx_handle* h, const int16_t* audio, int n_frames, float* grid, float* power);
/* the search on caller-supplied grids -> per frame f0_idx / h0_idx / score [max_cands] in output order and counts; best_score /
 * best_h0 (optional, [n_frames][f0_hi - f0_lo]): the per-bin maxima before threshold and neighbour suppression */
int  ft8rx_ft4_sync(ft8rx_handle* h, const float* grid, int n_frames, int32_t* f0_idx, int32_t* h0_idx, float* score, int32_t* counts,
                    float* best_score, int32_t* best_h0);
/* fine sync and demodulation of n (frame, f0, h0) triples -> tweak [n][2] = (dt / 36, df index), metric [n], llr [n][174], snr [n] */
int  ft8rx_ft4_demod(ft8rx_handle* h, const int16_t* audio, int n_frames, int n, const int32_t* frame, const int32_t* f0_idx,
                     const int32_t* h0_idx, int32_t* tweak, float* metric, float* llr, int32_t* snr);
/* Coherent LLRs (opt-in; k_ft4_coh; the twin is ft4.coherent_llrs).  on != 0: every FT4 batch enqueued
 * afterwards runs, on the candidates its BP left undecoded, the complex 105 x 4 amplitudes at the fine sync's winner, a residual-
 * frequency scan over q = -4 .. 4 x 0.651 Hz on the 16 sync symbols, max-log LLRs over runs of two and of four symbols, and the same BP
 * (bp_nc0_b, bp_iters_b, the handle's msg_types) on the run-of-2 rows, then on the run-of-4 rows; OSD follows on the single-symbol
 * LLRs of what is left.  Such a decode is a BP decode (ipass 4, FT8RX_M_LDPC_B, ap 0) whose record carries the run length in nsync
 * (2 or 4; every other FT4 record leaves nsync 0) and whose event carries slot 1 or 2.  Host state only, never refused; off (the
 * default): nothing new is launched or allocated, every byte is as before.  The workspaces (2.9 KB per candidate slot) are allocated
 * at the first FT4 batch that runs with the setting on, all or nothing; ft8rx_ft4_info's figure does not include them. */
int  ft8rx_ft4_set_coherent(ft8rx_handle* h, int32_t on);
/* bytes of coherent workspace the handle holds (0 until the first FT4 batch with the setting on) and the setting; either may be NULL */
int  ft8rx_ft4_coh_info(ft8rx_handle* h, uint64_t* workspace_bytes, int32_t* on);
/* stage entry point (tests): the chain's own launch on n caller-supplied candidates (frame, f0, h0) and fine-sync winners (ttweak in
 * -4 .. 4, ftweak in -2 .. 2) -> q [n], metrics [n][9], llr2 and llr4 [n][174] */
int  ft8rx_ft4_coherent(ft8rx_handle* h, const int16_t* audio, int n_frames, int n, const int32_t* frame, const int32_t* f0_idx,
                        const int32_t* h0_idx, const int32_t* ttweak, const int32_t* ftweak, int32_t* q, float* metrics, float* llr2,
                        float* llr4);
/* Weak search (opt-in; k_ft4_cgrid, k_ft4_csync; the twin is ft4.search_weak).  on != 0: every FT4 batch
 * enqueued afterwards finds its candidates by a coherent Costas sync on the 2.6042-Hz grid instead of the dB grid's search: per row
 * (12 ms) and carrier fq (x 12000 / 4608 Hz) the complex 576-sample sums of the four tones, the carrier's phase referred to sample 0 of
 * the frame; per (fq, h) the four Costas blocks' sums B_b, added as complex numbers inside a block, and
 *   score = (|B_0| + |B_1| + |B_2| + |B_3|) / sqrt(N),  N = the mean |sum|^2 over the 16 sync symbols and the 4 tones  (0 .. 32);
 * per bin f0 the first maximum over fq = 4 f0 - 2 .. 4 f0 + 1 and the h0 range.  The bins at or above weak_min (<= 0: the default)
 * that no neighbour beats are the candidates -- the same (f0_idx, h0_idx, score) records, max_cands, range and order as without it;
 * everything behind the list (fine sync, demodulator, BP, the coherent step, OSD, subtraction, reports) is untouched.  Host state only,
 * never refused; off (the default): nothing new is launched or allocated, every byte is as before.  The workspace (11.6 MB per frame of
 * max_frames: the grid, 628 rows x 2306 carriers) is allocated at the first FT4 batch that runs with the setting on, all or nothing;
 * ft8rx_ft4_info's figure does not include it. */
int  ft8rx_ft4_set_weak(ft8rx_handle* h, int32_t on, float weak_min);
/* bytes of weak-search workspace the handle holds (0 until the first FT4 batch with the setting on), the setting and its threshold;
 * any pointer may be NULL */
int  ft8rx_ft4_weak_info(ft8rx_handle* h, uint64_t* workspace_bytes, int32_t* on, float* weak_min);
/* stage entry point (tests): the chain's own launches on caller-supplied frames -> what ft8rx_ft4_sync returns (best / best_h0 optional) */
int  ft8rx_ft4_sync_weak(ft8rx_handle* h, const int16_t* audio, int n_frames, int32_t* f0_idx, int32_t* h0_idx, float* score,
                         int32_t* counts, float* best_score, int32_t* best_h0);
/* OSD on the coherent LLRs behind a whole-message score (opt-in; kernels/ft4_verify.hpp; the twin is
 * ft4.verify_score).  on != 0: every FT4 batch enqueued afterwards that runs the coherent step (ft8rx_ft4_set_coherent; without it the
 * setting does nothing) runs, behind the unchanged single-symbol OSD, OSD once more on the run-of-2 and the run-of-4 rows of every
 * candidate on OSD's list: the handle's order settings and msg_types, the distance gate max_hd (<= 0: the default).  A Hamming gate
 * alone cannot carry this step, so every word it returns is scored against the audio: with C the complex amplitudes of section 19.8,
 * turned by q, and T the word's 105 tones,
 *   score = A / sqrt(N),  A = sum over the 26 runs of four symbols from symbol 1 on of |sum C[s][T[s]]|,
 *                         N = the mean |C|^2 over symbols 1 .. 103 and the 4 tones     (0 where N = 0; near 206 on a clean signal).
 * A candidate the chain has decoded keeps its record byte for byte.  A candidate left EXHAUSTED becomes decoded by a word with
 * score >= min_score (<= 0: the default), run length 2 winning over 4: an OSD decode (ipass 5, FT8RX_M_OSD, ap 0, n_its = the trial,
 * osd_hd = the distance to that row's hard decisions) whose record carries the run length in nsync, rint(100 score) in pad2 and whose
 * event carries slot 1 or 2.  Host state only, never refused; off (the default): nothing new is launched or allocated, every byte is
 * as before.  The workspaces (1.4 KB per candidate slot) are allocated at the first FT4 batch that runs the step, all or nothing;
 * the figures of ft8rx_ft4_info, ft8rx_ft4_coh_info and ft8rx_ft4_weak_info do not include them.
 * Measured on an MI355X with these defaults (tools/ft4_measure.py --coh-osd, profiles/ft4_notes.md, section 19.11): no false decode on
 * 2048 noise frames behind either search, at msg_types 0 (77.1) and all (81.0); one wrong word (score 90.6) among the 1400 signals of
 * the decode table; 50 % decode probability at -15.9 dB instead of -15.7 (coherent alone), 44 instead of 28 of 200 signals at -17 dB
 * behind the weak search; 40.0 k instead of 40.8 k frames/s at B = 256 (the stage: 0.13 ms).  The defaults come from 14 noise words (22
 * at msg_types all): the gate is measured, but on a thin tail. */
#define FT8RX_FT4_COH_OSD_MIN_SCORE_DEFAULT 77.1f   /* S_max + (S_max - S_90) of the noise words within max_hd (76.84, 76.62), rounded up */
#define FT8RX_FT4_COH_OSD_MIN_SCORE_MSG_TYPES 81.0f /* the same from the noise words at msg_types all (79.27, 77.57): what Receiver takes then */
#define FT8RX_FT4_COH_OSD_MAX_HD_DEFAULT    40      /* the smallest multiple of 4 that keeps 99 % of the true words (all 71 lie in 17 .. 39) */
int  ft8rx_ft4_set_coh_osd(ft8rx_handle* h, int32_t on, float min_score, int32_t max_hd);
/* bytes of the step's workspace the handle holds (0 until the first FT4 batch that runs it), the setting and its two gates; any
 * pointer may be NULL */
int  ft8rx_ft4_coh_osd_info(ft8rx_handle* h, uint64_t* workspace_bytes, int32_t* on, float* min_score, int32_t* max_hd);
/* stage entry point (tests): the chain's own launch of k_ft4_verify on n caller-supplied candidates (frame, f0, h0), fine-sync
 * winners (ttweak in -4 .. 4, ftweak in -2 .. 2), residuals q in -4 .. 4 and 77-bit words -> score [n]; tones (optional): [n][105],
 * the words' tones as the kernel encoded them */
int  ft8rx_ft4_verify(ft8rx_handle* h, const int16_t* audio, int n_frames, int n, const int32_t* frame, const int32_t* f0_idx,
                      const int32_t* h0_idx, const int32_t* ttweak, const int32_t* ftweak, const int32_t* q, const uint64_t* msg_lo,
                      const uint64_t* msg_hi, float* score, uint8_t* tones);
/* ft8rx_ldpc / ft8rx_osd_ext on raw LLR vectors of FT4 codewords: the returned words are descrambled; mask = FT8RX_MT_* bits */
int  ft8rx_ft4_ldpc(ft8rx_handle* h, const float* llr, int n, int max_ncheck0, int max_iters, int32_t mask, int32_t* ok, uint64_t* msg_lo,
                    uint64_t* msg_hi, int32_t* n_its, int32_t* has_out, float* llr_out);
int  ft8rx_ft4_osd(ft8rx_handle* h, const float* llr, int n, int singleflips, int doubleflips, int tripleflips, int max_hd, int32_t mask,
                   int32_t* ok, uint64_t* msg_lo, uint64_t* msg_hi, int32_t* trial, int32_t* hd);
/* 77-bit words -> the 105 transmitted tones, [n][105].  Host function, no GPU. */
int  ft8rx_ft4_encode_tones(const uint64_t* msg_lo, const uint64_t* msg_hi, int n, uint8_t* tones);

/* ---- FT4 subtraction passes (extension; kernels/ft4_sub.hpp; pyft8_amd/ft4.py holds the float64 twin) ----
 * A decoded signal is its start sample (144 h0_idx + 36 ttweak, may be negative), the frequency of tone 0 as an integer in units of
 * 12000 / 4608 Hz (4 f0_idx + ftweak) and its 105 tones.  Its model s[n], n < 60480, is the complex form of the transmit waveform;
 * y[n] = x[start + n] conj(s[n]) (x = 0 outside the frame) is low-passed to the 41 bins k = -20 .. 20 of its 60480-point transform
 * (+-3.97 Hz) and x -= 2 Re(a s) with a the inverse transform of those bins.  No sample outside the frame is read or written. */
typedef struct {
    int32_t start;                   /* samples, may be negative */
    int32_t fq;                      /* tone 0 in units of 12000/4608 Hz, [0, 4608) */
    uint8_t tones[105];
    uint8_t pad[7];
} ft8rx_ft4_subsig;
/* For every frame, signals sigs[frame][0 .. counts[frame]) ([n_frames][max_sigs], max_sigs <= 256) are subtracted in list order from
 * a float32 working copy of the device-resident int16 frames (d_audio: a device pointer, [n_frames][90000]); the residual is rounded
 * back in place (rint, clipped).  refine = 0: the given starts; refine = 1: before a signal is subtracted the energy of its 41 bins is
 * evaluated at start + d, d = -24, -20 .. +24 samples, the first maximum wins and the start is written back into sigs; any other
 * value is refused.  audio_f32_out (host, optional, [n_frames][90000]): the float32 residual before rounding.  Synchronous.  The
 * workspaces (0.4 MB per frame of max_frames) are allocated at the first call of this or of ft8rx_ft4_sub_probe, all or nothing;
 * ft8rx_ft4_info's figure does not include them. */
int  ft8rx_ft4_subtract(ft8rx_handle* h, int16_t* d_audio, int n_frames, ft8rx_ft4_subsig* sigs, const int32_t* counts, int max_sigs,
                        int refine, float* audio_f32_out);
/* The signals a sweep removes: a frame's decoded FT4 records in emit order (BP decodes, then OSD's, each in score order), every 77-bit
 * word once, at its first occurrence, without the words the frame already has (have_lo / have_hi [n_frames][max_have] with
 * have_counts; NULL = none).  sigs: [n_frames][max_sigs]; returns the largest per-frame count (or < 0).  Host function, no GPU. */
int  ft8rx_ft4_subtraction_list(const ft8rx_record* records, const int32_t* counts, int max_cands, int n_frames, const uint64_t* have_lo,
                                const uint64_t* have_hi, const int32_t* have_counts, int max_have, ft8rx_ft4_subsig* sigs, int max_sigs,
                                int32_t* sig_counts);
/* bytes of FT4 subtraction workspace the handle holds (0 until its first ft8rx_ft4_subtract / ft8rx_ft4_sub_probe) */
int  ft8rx_ft4_sub_info(ft8rx_handle* h, uint64_t* workspace_bytes);
/* the handle's device buffer of FT4 frames ([max_frames][90000]; where the host entries leave the frames of a batch); NULL before the
 * handle's first FT4 call */
int16_t* ft8rx_ft4_staging_audio(ft8rx_handle* h);
/* stage entry point (tests): n signals, signal i on frame frame[i] of the host frames -> model (optional) [n][60480][2], the bins at
 * the given start [n][41][2] (index k + 20) and the energies of the 13 refine trials [n][13] */
int  ft8rx_ft4_sub_probe(ft8rx_handle* h, const int16_t* audio, int n_frames, int n, const int32_t* frame, const ft8rx_ft4_subsig* sigs,
                         float* model, double* bins, double* energy);

/* ---- FT4 measured reports (extension; kernels/ft4_report.hpp; pyft8_amd/ft4.py holds the float64 twin) ----
 * A decoded FT4 signal (ft8rx_ft4_subsig: start s0, fq, its 105 tones) is measured against its own model s[n], the subtraction's:
 * y_tau[n] = x[s0 + tau + n] conj(s[n]) for the trial starts tau = -36, -30 .. +36 samples, x = 0 outside [0, n_have), and on the
 * segment sums G_tau[j] = sum_{n < 36} y_tau[36 j + n], j < 1680:
 *   score[tau][delta] = sum over the blocks of four symbols {1..4}, {5..8} .. {97..100}, {101..103} of |sum_{q in block} C[q]|^2,
 *   C[q] = sum_{j < 16} G_tau[16 q + j] e^{-2 pi i delta (36 (16 q + j) + 17.5) / 12000}, delta = -6 .. +6 steps of 0.6510 Hz;
 *   the first maximum in tau-major order, a three-point parabola on each axis where the peak is interior (FT8RX_RP_EDGE_T / _F
 *   where it is not): t_sec = (s0 + tau + 6 dtau) / 12000, f_hz = fq 12000 / 4608 + delta, score = the maximum;
 *   snr_db = 10 log10(max(on / off - 1, 1e-3) * 20.8333 / 2500) at the peak's tau and the interpolated delta over the valid symbols
 *   (1 .. 103, their 576 samples wholly inside [0, n_have); fewer than 32: FT8RX_RP_INVALID and NaN fields): on = the mean |C[q]|^2,
 *   off = the lower quartile c[(m - 1) / 4] / ln(4/3) * 576 / 216 of the m Hann-weighted cells (w[n] = 1/2 - 1/2 cos(2 pi (n + 1/2) /
 *   576)) of the same samples at fq + 8 t, t = -5, -4, -3, 6, 7, 8, a frequency outside [8, 2296] dropped whole; off = 0 reads -50.79.
 * d_audio: a device pointer to [n_frames][90000] int16 (ft8rx_ft4_staging_audio after an FT4 batch); it is only read.  sigs
 * [n_frames][max_sigs] with counts [n_frames]; reports [n_frames][max_sigs]: FT8RX_RP_MEASURED on every measured slot, all zero from
 * counts[frame] on.  scores (optional) [n_frames][max_sigs][169], on_off (optional) [n_frames][max_sigs][2]: the stages (NaN on_off
 * with FT8RX_RP_INVALID).  Synchronous; a report is the same bytes alone or in a batch.  Refused by name before any launch: a tone
 * above 3, fq outside [0, 4608), |start| above 2^20, n_have outside [576, 90000], max_sigs below 1.  The workspaces (0.95 MB per
 * frame of max_frames) are allocated at the first call, all or nothing; the figures of ft8rx_ft4_info and ft8rx_ft4_sub_info do not
 * include them. */
int  ft8rx_ft4_report(ft8rx_handle* h, const int16_t* d_audio, int n_frames, const ft8rx_ft4_subsig* sigs, const int32_t* counts,
                      int max_sigs, int n_have, ft8rx_report* reports, float* scores, float* on_off);
/* bytes of FT4 report workspace the handle holds (0 until its first ft8rx_ft4_report) */
int  ft8rx_ft4_report_info(ft8rx_handle* h, uint64_t* workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
