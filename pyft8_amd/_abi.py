"""The C ABI of libft8rx.so as ctypes sees it: every function of include/ft8rx.h once, result type first, then the argument
types.  _lib.lib() applies the table to each build when it loads it; nothing else sets argtypes or restype on an ft8rx_ symbol.
tests/test_abi.py holds the table to the header: names, argument counts and type classes."""
import ctypes as C

PTR, STR, INT, I32, U64, F32 = C.c_void_p, C.c_char_p, C.c_int, C.c_int32, C.c_uint64, C.c_float
# PTR is any pointer but `const char*`: it takes byref(x), arr.ctypes.data, a ctypes array or pointer, c_void_p(p), an int and None alike

_RECS = (PTR, PTR, PTR, PTR)                       # records, counts, events, event_counts
_PKG = (PTR, INT, PTR, INT, PTR, PTR)              # out, max_msgs, out_counts, n_threads, table, flags
_FINE = (INT, (PTR, PTR, INT, INT) + (PTR,) * 11)
_SCORES = (INT, (PTR, PTR, INT, INT, INT, PTR, PTR))

PROTOTYPES = {
    # lifecycle
    "ft8rx_default_config": (INT, (PTR,)),
    "ft8rx_create": (INT, (PTR, INT, INT, PTR)),
    "ft8rx_destroy": (None, (PTR,)),
    "ft8rx_last_error": (STR, (PTR,)),
    "ft8rx_device_count": (INT, ()),
    "ft8rx_device_pci_bus_id": (INT, (INT, PTR, INT)),
    "ft8rx_build_info": (INT, (PTR, PTR, PTR)),
    "ft8rx_build_limits": (INT, (PTR, PTR)),
    "ft8rx_get_fft_plans": (INT, (PTR, PTR, PTR, PTR)),
    # whole path
    "ft8rx_decode_batch": (INT, (PTR, PTR, INT) + _RECS),
    "ft8rx_enqueue_batch": (INT, (PTR, PTR, INT)),
    "ft8rx_enqueue_batch_host": (INT, (PTR, PTR, INT)),
    "ft8rx_sync": (INT, (PTR,)),
    "ft8rx_fetch_results": (INT, (PTR, INT) + _RECS),
    "ft8rx_fetch_results_view": (INT, (PTR, INT) + _RECS),
    "ft8rx_results_to_device": (INT, (PTR, INT) + _RECS),
    "ft8rx_decode_messages": (INT, (PTR, PTR, INT) + _PKG),
    # float32 frames: the twins of the entries above and below
    "ft8rx_decode_batch_f32": (INT, (PTR, PTR, INT) + _RECS),
    "ft8rx_enqueue_batch_f32": (INT, (PTR, PTR, INT)),
    "ft8rx_enqueue_batch_host_f32": (INT, (PTR, PTR, INT)),
    "ft8rx_decode_messages_f32": (INT, (PTR, PTR, INT) + _PKG),
    "ft8rx_staging_audio_f32": (PTR, (PTR,)),
    "ft8rx_spectrogram_f32": (INT, (PTR, PTR, INT, PTR)),
    "ft8rx_cycle_spectrum_f32": (INT, (PTR, PTR, INT, PTR)),
    "ft8rx_ddc_stream_frame_f32": (INT, (PTR, U64, INT, PTR)),
    "ft8rx_subtract_f32": (INT, (PTR, PTR, INT, PTR, PTR, INT, INT, PTR)),
    # packed results
    "ft8rx_set_packed_output": (INT, (PTR, PTR, PTR, U64)),
    "ft8rx_packed_results": (INT, (PTR, PTR, PTR)),
    "ft8rx_packed_output_fence": (INT, (PTR, INT, PTR)),
    "ft8rx_package_packed": (INT, (PTR, U64, INT, INT) + _PKG),
    # tuning and service
    "ft8rx_set_streams": (INT, (PTR, INT)),
    "ft8rx_set_subbatch": (INT, (PTR, INT)),
    "ft8rx_set_ladder_mode": (INT, (PTR, INT)),
    "ft8rx_set_ladder_grid": (INT, (PTR, INT)),
    "ft8rx_set_search_mask": (INT, (PTR, PTR, INT)),
    "ft8rx_set_profiling": (INT, (PTR, INT)),
    "ft8rx_get_stage_times": (INT, (PTR, PTR, PTR, PTR)),
    "ft8rx_set_reject_log": (INT, (STR,)),
    "ft8rx_staging_audio": (PTR, (PTR,)),
    "ft8rx_copy_to_host": (INT, (PTR, PTR, PTR, U64)),
    "ft8rx_d2h_async": (INT, (PTR, PTR, PTR, U64, PTR)),
    "ft8rx_d2h_query": (INT, (PTR, I32)),
    "ft8rx_d2h_event": (PTR, (PTR, I32)),
    "ft8rx_alloc_host": (PTR, (PTR, U64)),
    "ft8rx_free_host": (INT, (PTR, PTR)),
    # opt-in steps
    "ft8rx_set_msg_types": (INT, (PTR, I32)),
    "ft8rx_set_weak": (INT, (PTR, I32, F32, I32)),
    "ft8rx_set_ap_calls": (INT, (PTR, STR, STR)),
    "ft8rx_set_ap_max_hd": (INT, (PTR, I32)),
    "ft8rx_ap_patterns": (INT, (STR, STR, PTR, PTR)),
    "ft8rx_ap_calls_probe": (INT, (PTR, PTR, INT, PTR, PTR, PTR)),
    "ft8rx_set_recall": (INT, (PTR, PTR, PTR, INT)),
    "ft8rx_fetch_recall": (INT, (PTR, INT, PTR, PTR)),
    "ft8rx_set_recall_gates": (INT, (PTR, I32, I32)),
    "ft8rx_recall_hypotheses": (INT, (PTR, PTR, PTR)),
    "ft8rx_recall_probe": (INT, (PTR, PTR, PTR, INT, PTR)),
    "ft8rx_set_reports": (INT, (PTR, I32)),
    "ft8rx_fetch_reports": (INT, (PTR, INT, PTR)),
    "ft8rx_report_probe": (INT, (PTR, PTR, INT, INT) + (PTR,) * 8),
    # down-converter
    "ft8rx_ddc": (INT, (PTR, PTR, INT, I32, INT, U64, U64, INT, PTR, PTR, F32, PTR, PTR, PTR)),
    "ft8rx_ddc_host": (INT, (PTR, PTR, INT, I32, INT, U64, U64, INT, PTR, PTR, F32, PTR)),
    "ft8rx_ddc_taps": (INT, (I32, INT, PTR, INT)),
    "ft8rx_ddc_stream_open": (INT, (PTR, INT, I32, INT, INT, PTR, PTR, F32, U64, INT, PTR)),
    "ft8rx_ddc_stream_push": (INT, (PTR, PTR, U64, INT, PTR)),
    "ft8rx_ddc_stream_frame": (INT, (PTR, U64, INT, PTR)),
    "ft8rx_ddc_stream_frames": (INT, (PTR, U64, INT, INT, PTR, INT, PTR)),
    "ft8rx_ddc_stream_read": (INT, (PTR, U64, INT, PTR, PTR)),
    "ft8rx_ddc_stream_info": (INT, (PTR, PTR, PTR, PTR, PTR)),
    "ft8rx_ddc_stream_close": (INT, (PTR,)),
    "ft8rx_ddc_stream_grid_open": (INT, (PTR, INT, INT)),
    "ft8rx_ddc_stream_grid_info": (INT, (PTR, PTR, PTR, PTR, PTR)),
    "ft8rx_ddc_stream_grid_read": (INT, (PTR, U64, INT, PTR)),
    "ft8rx_ddc_wide_plan": (INT, (I32, PTR, PTR)),
    "ft8rx_ddc_wide_taps": (INT, (I32, PTR, INT)),
    "ft8rx_ddc_wide": (INT, (PTR, PTR, INT, I32, U64, INT, PTR, F32, PTR, PTR, PTR)),
    "ft8rx_ddc_wide_host": (INT, (PTR, PTR, INT, I32, U64, INT, PTR, F32, PTR)),
    "ft8rx_ddc_wide_stream_open": (INT, (PTR, INT, I32, INT, PTR, F32, U64, INT, PTR)),
    "ft8rx_ddc_wide_stream_push": (INT, (PTR, PTR, U64, INT, PTR)),
    "ft8rx_ddc_wide_stream_read_mid": (INT, (PTR, U64, INT, PTR)),
    "ft8rx_ddc_wide_stream_close": (INT, (PTR,)),
    "ft8rx_ddc_rat_plan": (INT, (I32, PTR, PTR, PTR, PTR)),
    "ft8rx_ddc_rat_taps": (INT, (I32, PTR, INT)),
    "ft8rx_ddc_rat": (INT, (PTR, PTR, INT, I32, U64, INT, PTR, F32, PTR, PTR, PTR)),
    "ft8rx_ddc_rat_host": (INT, (PTR, PTR, INT, I32, U64, INT, PTR, F32, PTR)),
    "ft8rx_ddc_rat_stream_open": (INT, (PTR, INT, I32, INT, PTR, F32, U64, INT, PTR)),
    "ft8rx_ddc_rat_stream_push": (INT, (PTR, PTR, U64, INT, PTR)),
    "ft8rx_ddc_rat_stream_read_mid": (INT, (PTR, U64, INT, PTR)),
    "ft8rx_ddc_rat_stream_close": (INT, (PTR,)),
    # noise blanker
    "ft8rx_blank": (INT, (PTR, PTR, INT, I32, INT, INT, PTR, PTR)),
    "ft8rx_blank_host": (INT, (PTR, PTR, INT, I32, INT, INT, PTR)),
    "ft8rx_blank_taper": (INT, (INT, PTR, INT)),
    # input-rate noise blanker
    "ft8rx_blank_in": (INT, (PTR, PTR, INT, U64, INT, I32, INT, INT, PTR, PTR, PTR)),
    "ft8rx_blank_in_host": (INT, (PTR, PTR, INT, U64, INT, I32, INT, INT, PTR, PTR)),
    "ft8rx_blank_in_stream_open": (INT, (PTR, INT, INT, I32, INT, INT, U64, U64)),
    "ft8rx_blank_in_stream_push": (INT, (PTR, PTR, U64, INT, INT, PTR, PTR, PTR)),
    "ft8rx_blank_in_stream_info": (INT, (PTR, PTR, PTR, PTR)),
    "ft8rx_blank_in_stream_close": (INT, (PTR,)),
    "ft8rx_blank_in_released": (INT, (U64, U64, INT, INT, INT, PTR)),
    # panorama
    "ft8rx_pan_window": (INT, (INT, PTR, INT)),
    "ft8rx_pan_rows_done": (INT, (U64, U64, INT, INT, PTR)),
    "ft8rx_pan": (INT, (PTR, PTR, INT, U64, INT, INT, PTR, PTR, PTR)),
    "ft8rx_pan_host": (INT, (PTR, PTR, INT, U64, INT, INT, PTR, PTR, PTR)),
    "ft8rx_pan_stream_open": (INT, (PTR, INT, INT, INT, INT, U64, U64)),
    "ft8rx_pan_stream_push": (INT, (PTR, PTR, U64, INT, PTR, PTR)),
    "ft8rx_pan_stream_read": (INT, (PTR, U64, INT, PTR, PTR)),
    "ft8rx_pan_stream_info": (INT, (PTR, PTR, PTR, PTR, PTR)),
    "ft8rx_pan_stream_close": (INT, (PTR,)),
    # stage entry points
    "ft8rx_spectrogram": (INT, (PTR, PTR, INT, PTR)),
    "ft8rx_hop_spectrum": (INT, (PTR, PTR, PTR)),
    "ft8rx_sync_search": (INT, (PTR, PTR, INT, PTR, PTR, PTR, PTR)),
    "ft8rx_sync_scores": _SCORES,
    "ft8rx_sync_scores_weak": _SCORES,
    "ft8rx_llr_grid": (INT, (PTR, PTR, INT, INT) + (PTR,) * 6),
    "ft8rx_cycle_spectrum": (INT, (PTR, PTR, INT, PTR)),
    "ft8rx_fine": _FINE,
    "ft8rx_fine_weak": _FINE,
    "ft8rx_ldpc": (INT, (PTR, PTR, INT, INT, INT) + (PTR,) * 6),
    "ft8rx_osd": (INT, (PTR, PTR, INT, INT, INT, PTR, PTR, PTR, PTR)),
    "ft8rx_osd_ext": (INT, (PTR, PTR, INT, INT, INT, INT, INT) + (PTR,) * 5),
    "ft8rx_crc_valid": (INT, (PTR, PTR, INT, PTR, PTR, PTR)),
    "ft8rx_valid77": (INT, (PTR, PTR, PTR, INT, PTR)),
    "ft8rx_valid77_ext": (INT, (PTR, PTR, PTR, INT, I32, PTR)),
    "ft8rx_math_probe": (INT, (PTR, INT, PTR, INT, PTR)),
    # workload generator, subtraction
    "ft8rx_synth_frames": (INT, (PTR, U64, INT, INT, INT, PTR, INT, PTR, PTR)),
    "ft8rx_synth_frames_ex": (INT, (PTR, U64, INT, INT, INT, PTR, INT, PTR, PTR, INT)),
    "ft8rx_subtract": (INT, (PTR, PTR, INT, PTR, PTR, INT, INT, PTR)),
    "ft8rx_subtraction_list": (INT, (PTR, PTR, INT, PTR, INT, INT, INT, PTR, INT, PTR)),
    "ft8rx_encode_tones": (INT, (PTR, PTR, INT, PTR)),
    # FT4 (7.5-s frames)
    "ft8rx_ft4_decode_batch": (INT, (PTR, PTR, INT) + _RECS),
    "ft8rx_ft4_enqueue_batch": (INT, (PTR, PTR, INT)),
    "ft8rx_ft4_set": (INT, (PTR, F32, I32)),
    "ft8rx_ft4_set_range": (INT, (PTR, I32, I32, I32, I32)),
    "ft8rx_ft4_info": (INT, (PTR, PTR, PTR, PTR, PTR)),
    "ft8rx_ft4_decode_messages": (INT, (PTR, PTR, INT) + _PKG),
    "ft8rx_ft4_grid": (INT, (PTR, PTR, INT, PTR, PTR)),
    "ft8rx_ft4_sync": (INT, (PTR, PTR, INT) + (PTR,) * 6),
    "ft8rx_ft4_demod": (INT, (PTR, PTR, INT, INT) + (PTR,) * 7),
    "ft8rx_ft4_set_coherent": (INT, (PTR, I32)),
    "ft8rx_ft4_coh_info": (INT, (PTR, PTR, PTR)),
    "ft8rx_ft4_coherent": (INT, (PTR, PTR, INT, INT) + (PTR,) * 9),
    "ft8rx_ft4_set_weak": (INT, (PTR, I32, F32)),
    "ft8rx_ft4_weak_info": (INT, (PTR, PTR, PTR, PTR)),
    "ft8rx_ft4_sync_weak": (INT, (PTR, PTR, INT) + (PTR,) * 6),
    "ft8rx_ft4_set_coh_osd": (INT, (PTR, I32, F32, I32)),
    "ft8rx_ft4_coh_osd_info": (INT, (PTR, PTR, PTR, PTR, PTR)),
    "ft8rx_ft4_verify": (INT, (PTR, PTR, INT, INT) + (PTR,) * 10),
    "ft8rx_ft4_ldpc": (INT, (PTR, PTR, INT, INT, INT, I32) + (PTR,) * 6),
    "ft8rx_ft4_osd": (INT, (PTR, PTR, INT, INT, INT, INT, INT, I32) + (PTR,) * 5),
    "ft8rx_ft4_encode_tones": (INT, (PTR, PTR, INT, PTR)),
    "ft8rx_ft4_subtract": (INT, (PTR, PTR, INT, PTR, PTR, INT, INT, PTR)),
    "ft8rx_ft4_subtraction_list": (INT, (PTR, PTR, INT, INT, PTR, PTR, PTR, INT, PTR, INT, PTR)),
    "ft8rx_ft4_staging_audio": (PTR, (PTR,)),
    "ft8rx_ft4_sub_info": (INT, (PTR, PTR)),
    "ft8rx_ft4_sub_probe": (INT, (PTR, PTR, INT, INT, PTR, PTR, PTR, PTR, PTR)),
    "ft8rx_ft4_report": (INT, (PTR, PTR, INT, PTR, PTR, INT, INT, PTR, PTR, PTR)),
    "ft8rx_ft4_report_info": (INT, (PTR, PTR)),
    # host message layer
    "ft8rx_package_batch": (INT, _RECS + (INT, INT) + _PKG),
    "ft8rx_package_batch_ext": (INT, _RECS + (INT, INT) + _PKG + (I32,)),
    "ft8rx_package_batch_recall": (INT, _RECS + (PTR, PTR, INT, INT) + _PKG),
    "ft8rx_merge_messages": (INT, (PTR, PTR, INT, PTR, PTR, INT, INT, INT, INT, PTR, PTR)),
    "ft8rx_hashes_create": (PTR, ()),
    "ft8rx_hashes_destroy": (None, (PTR,)),
    "ft8rx_hashes_clear": (INT, (PTR,)),
    "ft8rx_hashes_add": (INT, (PTR, STR)),
    "ft8rx_hashes_size": (INT, (PTR,)),
}

# defined in csrc/ft8rx.hip, not in the header, and exported by the timing-only builds alone (tools/{fine,bp,osd}_timing.py):
# declared where the loaded library has them
OPTIONAL = {name: (INT, (PTR, PTR, INT)) for name in ("ft8rx_debug_fine_times", "ft8rx_debug_bp_times", "ft8rx_debug_osd_times")}


def declare(L, prototypes=PROTOTYPES, optional=OPTIONAL):
    """Set restype / argtypes of every table entry on the loaded library L -> the names of `prototypes` that L does not export."""
    missing = []
    for table, required in ((prototypes, True), (optional, False)):
        for name, (res, args) in table.items():
            fn = getattr(L, name, None)
            if fn is None:
                if required:
                    missing.append(name)
                continue
            fn.restype, fn.argtypes = res, list(args)
    return missing
