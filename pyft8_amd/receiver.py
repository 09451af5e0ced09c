"""Drop-in surface of PyFT8/receiver.py for the MI355X build: batched, frame-complete decoding.

    Receiver(input_device_keywords, on_message, sync_score_min=85, max_cands=200,
             search_freq_range=[100,3000], search_time_range=[-2.0,3.0], verbose=False)   reference receiver.py:310-336
      .audio_in.search_grid / .waterfall_data / .get_cycle_spectrum()                    reference receiver.py:225-306
      .search(cyclestart_string, odd_even, search_f_idxs) -> [Candidate]                  reference receiver.py:338-367
      .set_band(band)                                                                     reference receiver.py:369
      .decode_frames(audio_i16[B,180000]) -> list[list[message dict]]                     (batch entry)
    decode_frames(audio, **receiver_kwargs)                                               module-level convenience

The reference is a real-time, one-frame-per-15-s receiver driven by PortAudio; this build decodes whole
frames ("frame-complete" semantics) in batches on the GPU.  Messages are delivered through
`on_message(dict)` with the reference's keys, on the caller's thread, in the reference's emit order.
There is no CPU path: without libft8rx.so and an MI355X the constructor raises.

Live use: like the reference, the constructor starts the receiver when an audio source exists -- PortAudio through
PyAudio if that module is importable (reference receiver.py:252, 266-270), or any iterator of 480-sample int16 hops passed as
`audio_source` -- plus a daemon thread that stands in for Receiver.manage_cycle (receiver.py:336, 372-412): it wakes every 0.1 s on
the `time_source` / `sleep` seam (time_utils.py:7-14) and decodes every completed cycle (poll()).  `Receiver.start()` / `.stop()`
do the same explicitly.

Noise blanker (extension): Receiver(..., noise_blanker=True | k | {"threshold": k, "guard": G, "taper": R}) blanks
impulses in every frame that is about to be decoded -- decode_frames / decode_frames_arrays, decode_stream, the live passes of poll --
on the GPU (ft8rx_blank) and leaves the per-frame counters of the last batch in `blanker_stats`.  The live `audio_in.search_grid` /
`waterfall_data`, and search() on them, stay the unblanked audio.  Off (the default) nothing of it runs.

Input blanker (extension): Receiver(..., input_blanker=True | k | {"threshold": k, "guard": G, "taper": R,
"block": B}), and the same keyword on decode_stream, blanks ONE stream of integer samples at its own rate on the GPU (ft8rx_blank_in*)
in front of the down-converter, which reads the blanked samples on the device; `input_blanker_stats` holds the cumulative counters.
The live search grid / waterfall of the channels show the blanked input.  Off (the default) nothing of it runs.

Panorama (extension): Receiver(..., sample_rate=..., panorama=True | {"n_fft", "n_avg" or "period_s", "rows"}),
and the same keyword on decode_stream, keeps the averaged power spectrum of ONE raw input stream at its own rate and the count of
samples at the converter's rails (ft8rx_pan*), computed on the GPU from the samples the front end reads; `panorama` holds the rows,
their statistics and the frequency axis.  Off (the default) nothing of it runs.

Float frames (extension): float_frames=True -- on decode_frames / decode_frames_arrays / decode_frame with float32
or float64 arrays, on decode_stream, or on Receiver(..., sample_rate=...) for the wide live input -- decodes unrounded float32 audio
end to end: the level of the input no longer matters and no gain has to be chosen.  Off (the default) nothing changes: float arrays
are refused as before.  noise_blanker, integer arithmetic on int16 by definition, is refused together with it.
"""
import threading as _threading
import time as _time

import numpy as np

from . import _lib
from . import blanker as _blanker
from . import ft4 as _ft4
from . import messages as _m
from . import optins as _optins
from . import pan as _pan
from . import wide_in as _wide_in

T_CYC, SYM_RATE, SAMP_RATE = 15, 6.25, 12000
WATERFALL_DOWNSAMPLE = 2


def config_from_kwargs(sync_score_min=85, max_cands=200, search_freq_range=(100, 3000), search_time_range=(-2.0, 3.0), **ext):
    """Receiver kwargs -> ft8rx_config (index arithmetic of reference receiver.py:233-235, 319)."""
    df = SYM_RATE / 2
    cfg = _lib.default_config(
        sync_score_min=float(sync_score_min), max_cands=int(min(max_cands, 1 << 30)),
        f0_lo=int(search_freq_range[0] / df), f0_hi=int(search_freq_range[1] / df),
        h0_lo=int((search_time_range[0] + 0.5) * 4 * SYM_RATE), h0_hi=int((search_time_range[1] + 0.5) * 4 * SYM_RATE))
    # The reference takes any value here (receiver.py:311-313, 319, 366-367); this build has compile-time layouts.  Say which
    # kwarg is out of range instead of letting ft8rx_create answer "configuration out of the supported range" (include/ft8rx.h).
    if cfg.max_cands < 1:
        raise _lib.Ft8rxError(f"max_cands={max_cands}: at least one candidate per frame")
    # max_cands: no limit.  Receiver.search makes at most one candidate per f0 bin (receiver.py:341-365), so any value beyond the
    # number of bins of the search range keeps exactly the same list, and both builds take that many (FT8RX_MAX_CANDS = 1024 > 956
    # bins up to 3000 Hz; libft8rx_wide.so: 2048 > 1884 bins of the widest range).
    cfg.max_cands = min(cfg.max_cands, max(1, cfg.f0_hi - cfg.f0_lo))
    # search_time_range: any window the reference itself can search.  Its search reads grid rows h0 + 148 .. h0 + 172 of a 750-row grid
    # (receiver.py:322, 346-347; negative rows wrap, rows >= 750 are an IndexError), i.e. h0 in [-898, 577]; candidates whose middle
    # Costas block leaves the fine-sync series (h0 outside [-140, 220]: beyond -6.1 .. +8.3 s) are scored in the time domain with
    # clamped reads, as the reference does (kernels/fine_sync.hpp: k_fine_td).
    if cfg.h0_lo < _lib.MIN_H0 or cfg.h0_hi > _lib.MAX_H0 or cfg.h0_hi <= cfg.h0_lo:
        raise _lib.Ft8rxError(f"search_time_range={list(search_time_range)}: a non-empty window inside [{_lib.MIN_H0 / 25 - 0.5:.1f}, "
                              f"{_lib.MAX_H0 / 25 - 0.5:.2f}] s (FT8RX_MIN_H0 / FT8RX_MAX_H0: beyond it the reference's own search indexes "
                              "outside its 750-row grid, receiver.py:346-347; its default is [-2, 3])")
    if cfg.f0_lo < 4 or cfg.f0_hi > _lib.MAX_F0_WIDE or cfg.f0_lo >= cfg.f0_hi:
        raise _lib.Ft8rxError(f"search_freq_range={list(search_freq_range)}: supported are 12.5 .. {_lib.MAX_F0_WIDE * df:.0f} Hz, low < high "
                              "(above 3000 Hz the wide build libft8rx_wide.so is used; the reference fails beyond ~5940 Hz, receiver.py:181-182)")
    mask = msg_types_mask(ext.pop("msg_types", 0))       # a handle setting, not a field of ft8rx_config (_lib.Config.msg_types)
    my_call, dx_call, ap_max_hd = ext.pop("my_call", None), ext.pop("dx_call", None), ext.pop("ap_max_hd", None)
    weak, weak_sync_min, weak_osd_max_hd = bool(ext.pop("weak", False)), ext.pop("weak_sync_min", None), ext.pop("weak_osd_max_hd", None)
    known = {f[0] for f in _lib.Config._fields_}
    for k, v in ext.items():          # extension knobs: bp_iters_b, osd_single, osd_double, osd_triple, osd_max_hd, ...
        if k not in known:            # like the reference's fixed signature (e.g. the CLI's misspelt `search_timerange`, pyft8.py:137)
            raise TypeError(f"Receiver() got an unexpected keyword argument '{k}'")
        setattr(cfg, k, v)
    if mask:
        cfg.msg_types = mask
    if ap_max_hd is not None:
        if not 1 <= int(ap_max_hd) <= 174:
            raise _lib.Ft8rxError(f"ap_max_hd={ap_max_hd}: a Hamming distance in 1 .. 174")
        cfg.ap_max_hd = int(ap_max_hd)
    set_ap_calls_cfg(cfg, my_call, dx_call)
    set_weak_cfg(cfg, weak, weak_sync_min, weak_osd_max_hd)
    return cfg


def set_weak_cfg(cfg, weak, sync_min=None, osd_max_hd=None):
    """Check the weak-mode kwargs (ft8rx_set_weak) and store them in cfg; refuses what optins.py excludes."""
    if not weak:
        if sync_min is not None or osd_max_hd is not None:
            raise _lib.Ft8rxError("weak_sync_min / weak_osd_max_hd need weak=True")
        return
    _optins.refuse(_optins.WEAK, _optins.active(cfg))
    if sync_min is not None and not (np.isfinite(float(sync_min)) and float(sync_min) > 0):
        raise _lib.Ft8rxError(f"weak_sync_min={sync_min}: a positive three-block Costas score")
    if osd_max_hd is not None and not 1 <= int(osd_max_hd) <= 174:
        raise _lib.Ft8rxError(f"weak_osd_max_hd={osd_max_hd}: a Hamming distance in 1 .. 174")
    cfg.weak = True
    cfg.weak_sync_min = None if sync_min is None else float(sync_min)
    cfg.weak_osd_max_hd = None if osd_max_hd is None else int(osd_max_hd)


def set_ap_calls_cfg(cfg, my_call, dx_call):
    """Check the a-priori calls (ft8rx_set_ap_calls: standard callsigns only) and store them in cfg; refuses what optins.py excludes."""
    my_call, dx_call = (my_call or None), (dx_call or None)
    if my_call or dx_call:
        _optins.refuse(_optins.AP_CALLS, _optins.active(cfg))
    _lib.ap_patterns(my_call, dx_call)                   # raises, naming the argument, for a call that is not a standard one
    cfg.ap_my_call, cfg.ap_dx_call = my_call, dx_call


def msg_types_mask(msg_types):
    """The msg_types kwarg (opt-in message types the reference leaves unimplemented; include/ft8rx.h FT8RX_MT_*) -> its bit mask:
    an int, "all", or a collection of names from {"free_text", "dxpedition", "field_day", "telemetry", "rtty_ru", "eu_vhf"}."""
    if isinstance(msg_types, str):
        if msg_types != "all":
            raise _lib.Ft8rxError(f'msg_types={msg_types!r}: "all", a set of {sorted(_lib.MSG_TYPE_BITS)} or an int bit mask')
        return _lib.MT_ALL
    if isinstance(msg_types, (int, np.integer)) and not isinstance(msg_types, bool):
        if not 0 <= int(msg_types) <= _lib.MT_ALL:
            raise _lib.Ft8rxError(f"msg_types={msg_types}: a bit mask in 0 .. {_lib.MT_ALL}")
        return int(msg_types)
    names = set(msg_types)
    bad = names - set(_lib.MSG_TYPE_BITS)
    if bad:
        raise _lib.Ft8rxError(f"msg_types: unknown message type(s) {sorted(bad)}; known are {sorted(_lib.MSG_TYPE_BITS)}")
    mask = 0
    for n in names:
        mask |= _lib.MSG_TYPE_BITS[n]
    return mask


def frames_from_ragged(frames):
    """Ragged input -> int16 [B, 180000].  `frames` is an array [B, n] / [n] or a list of 1-D arrays, each at most 15 s long;
    shorter frames are padded with digital silence at the end (the reference's ring buffer is zero before the first hop,
    receiver.py:248; in frame-complete semantics the frame starts at cycle time 0, so the missing tail is what is silent).
    Longer input is an error: cut a recording into cycles yourself -- the cycle boundary is yours to choose."""
    if isinstance(frames, np.ndarray) and frames.ndim == 1:
        frames = [frames]
    out = np.zeros((len(frames), _lib.NSAMP), np.int16)
    for i, f in enumerate(frames):
        f = np.asarray(f)
        if f.ndim != 1:
            raise _lib.Ft8rxError(f"frame {i}: expected a 1-D array of int16 samples, got shape {f.shape}")
        if f.dtype != np.int16:
            if not np.issubdtype(f.dtype, np.integer):
                raise _lib.Ft8rxError(f"frame {i}: samples must be integers in int16 range (got {f.dtype})")
            if len(f) and (f.min() < -32768 or f.max() > 32767):
                raise _lib.Ft8rxError(f"frame {i}: samples outside the int16 range")
        if len(f) > _lib.NSAMP:
            raise _lib.Ft8rxError(f"frame {i}: {len(f)} samples > {_lib.NSAMP} (15 s at 12 kHz)")
        out[i, :len(f)] = f
    return out


def frames_from_ragged_f32(frames):
    """frames_from_ragged for float frames (float_frames=True): float32 / float64 input -> float32 [B, 180000],
    float64 rounded to float32 once, shorter frames padded with zeros at the end.  Any other dtype, a longer frame and a non-finite
    value (NaN, infinity: named with the frame) are refused."""
    if isinstance(frames, np.ndarray) and frames.ndim == 1:
        frames = [frames]
    out = np.zeros((len(frames), _lib.NSAMP), np.float32)
    for i, f in enumerate(frames):
        f = np.asarray(f)
        if f.ndim != 1:
            raise _lib.Ft8rxError(f"frame {i}: expected a 1-D array of float samples, got shape {f.shape}")
        if f.dtype not in (np.float32, np.float64):
            raise _lib.Ft8rxError(f"frame {i}: float_frames=True takes float32 or float64 samples (got {f.dtype})")
        if len(f) > _lib.NSAMP:
            raise _lib.Ft8rxError(f"frame {i}: {len(f)} samples > {_lib.NSAMP} (15 s at 12 kHz)")
        with np.errstate(over="ignore"):
            out[i, :len(f)] = f                                   # float64 -> float32: one rounding
        if not np.isfinite(out[i, :len(f)]).all():
            raise _lib.Ft8rxError(f"frame {i}: non-finite samples (NaN or infinity, or a float64 beyond the float32 range)")
    return out


def refuse_float_with_blanker(float_frames, noise_blanker):
    """noise_blanker is the one opt-in float frames refuse (DESIGN.md sections 15, 18)"""
    if float_frames and noise_blanker is not None:
        raise _lib.Ft8rxError("float_frames=True is not supported together with noise_blanker: its definition is integer arithmetic on "
                              "int16 frames (input_blanker, in front of the down-converter, stays allowed)")


# AP masks of the reference (receiver.py:21-27), as data: (name, first bit, forced bit values); 'CQ' also forces bits 74, 75 -> 0,
# 76 -> 1 and 57, 58 -> 0 (:113-116).  The 'RR73' mask is the reference's, quirk included.
AP_PATTERNS = (("NoAP", 0, ""), ("CQ", 0, "00000000000000000000000000100"), ("RR73", 58, "0111111001110101001"),
               ("73", 58, "0111111010010100001"), ("RRR", 58, "0111111010010010001"))
# the ipass ladder (receiver.py:68-107): step -> (attempt, AP variants, arguments)
def _weak_osd_max_hd(cfg):
    """The OSD distance gate of weak mode: an explicit config.osd_max_hd wins over the setting's (ft8rx.hip: weak_config)."""
    if cfg.osd_max_hd:
        return int(cfg.osd_max_hd)
    return _lib.WEAK_OSD_MAX_HD_DEFAULT if cfg.weak_osd_max_hd is None else int(cfg.weak_osd_max_hd)


_LADDER = {0: ("good91+ldpc", range(5), (35, 5, False)), 2: ("good91", range(2), None), 3: ("ldpc", range(2), (35, 5, False)),
           4: ("ldpc", range(5), (90, 20, True)), 5: ("osd", range(5), None)}


def frames_from_wav(path, cycle_offset_s=0.0):
    """A mono 16-bit 12 kHz .wav (what the reference's pipeline scripts read with the `wave` module, tests/pipeline/*.py; its two
    fixture recordings) -> int16 [n_frames, 180000]: the recording cut into consecutive 15-s cycles from `cycle_offset_s` on, the
    last one padded with digital silence (frames_from_ragged).  Anything else than mono / 16 bit / 12 kHz is rejected -- resampling
    is not this package's business."""
    import wave
    with wave.open(path, "rb") as w:
        if (w.getnchannels(), w.getsampwidth(), w.getframerate()) != (1, 2, SAMP_RATE):
            raise _lib.Ft8rxError(f"{path}: need mono 16-bit {SAMP_RATE} Hz, got {w.getnchannels()} ch / {8 * w.getsampwidth()} bit / {w.getframerate()} Hz")
        x = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    x = x[int(round(cycle_offset_s * SAMP_RATE)):]
    if len(x) == 0:
        return np.zeros((0, _lib.NSAMP), np.int16)
    return frames_from_ragged([x[i:i + _lib.NSAMP] for i in range(0, len(x), _lib.NSAMP)])


def ap_calls_attempts(h, cfg, llr, bits, mask, max_hd, lock, synth, met=None):
    """ipass 7 of one candidate's fine LLRs `llr` with the patterns (bits, mask) of _lib.ap_patterns, on handle h, by the rule of
    kernels/ap_calls.hpp: partial patterns (5..7) BP(bp_nc0_b, bp_iters_b) on the overridden LLRs, and OSD only if BP found no valid
    word (not for a vector with a NaN); full ones (8..10) a codeword test; each accepted only within max_hd of the hard decisions of
    `llr`.  -> (ap, 77-bit word, distance, method) of the smallest distance (ties: pattern order), or None.  met (a list): gets the
    (ap, word) of every valid word the attempts meet, in the batch's event order (accepted or not; a codeword only when accepted)."""
    llr = np.asarray(llr, np.float32)
    hard = (llr > 0).astype(np.uint8)
    best = None
    for k in range(6):
        if not mask[k].any():
            continue
        ap = 5 + k
        if ap >= 8:
            hd = int((bits[k] != hard).sum())
            word = int("".join(str(int(b)) for b in bits[k][:77]), 2)
            res = (word, hd, _lib.M_AP_CODEWORD)
            if hd > max_hd:
                continue
        else:
            x = np.where(mask[k] == 1, np.where(bits[k] == 1, 5.0, -5.0), llr).astype(np.float32)[None]
            with lock:
                ok, lo, hi, _, _, _ = h.ldpc(x, cfg.bp_nc0_b, cfg.bp_iters_b)
                method = _lib.M_LDPC_B
                if not ok[0] and not np.isnan(x).any():
                    ok, lo, hi, _ = h.osd(x, cfg.osd_single, cfg.osd_double, cfg.osd_triple)
                    method = _lib.M_OSD
            if not ok[0]:
                continue
            word = (int(hi[0]) << 64) | int(lo[0])
            cw = synth.encode174(word)
            hd = int(sum(((cw >> (173 - i)) & 1) != hard[i] for i in range(174)))
            res = (word, hd, method)
        if met is not None:
            met.append((ap, word))
        if res[1] <= max_hd and (best is None or res[1] < best[2]):
            best = (ap, res[0], res[1], res[2])
    return best


class Candidate:
    """One sync candidate (reference receiver.py:29-135): `origin`, `search_grid_bounds`, and -- for candidates returned by
    Receiver.search -- the reference's per-candidate state machine: decode(current_max_ipass) advances ONE ladder step per call
    (:68-107) and check_and_package(duplicate_filter) emits the message dict (:51-66).  Every step runs on the GPU through the
    stage entry points (ft8rx_llr_grid, ft8rx_fine, ft8rx_ldpc, ft8rx_osd, ft8rx_crc_valid); batched decoding
    (Receiver.decode_frames) does not go through this class -- it exists so that code written against the reference's
    Candidate API (the manage_cycle loop, tests/pipeline scripts) runs unchanged."""

    def __init__(self, origin, search_grid_bounds, record=None, rx=None, grid=None, llr_sd_min=5):
        self.origin = origin
        self.search_grid_bounds = search_grid_bounds
        self.record = record
        self.decode_result = None
        self._rx, self._grid = rx, grid
        self.on_message = rx.on_message if rx is not None else None
        self.llr_sd, self.llr_sd_min = 0, llr_sd_min
        self.ipass = 0
        self.source = None
        self.tweaks = "t:%+03d f:%+03d" % (0, 0)
        self.saved_llrs = []
        self.n_sync_matches = 100
        self.decode_notes = ""
        self.snr = 0
        self._tt = self._ft = 0              # the fine tweaks as numbers (0 until the fine stage has accepted the candidate)

    # ---- receiver.py:51-66
    def check_and_package(self, duplicate_filter):
        self.msg_text = " ".join(self.decode_result)
        o = self.origin
        key = o["cyclestart_string"] + self.msg_text
        if key not in duplicate_filter:
            duplicate_filter.add(key)
            snr = "%+03d" % self.snr
            message = {"band": o["band"], "tsec": o["tsec"], "fHz": o["fHz"], "msg_tuple": self.decode_result, "their_snr": snr,
                       "their_tx_cycle": o["odd_even"],
                       "all_txt_format": f"{o['cyclestart_string']} {snr} {(o['tsec'] - 0.6):4.1f} {o['fHz']:4.0f} ~ {self.msg_text}",
                       "cyclestart_string": o["cyclestart_string"], "decode_completed": self._rx.time_source() if self._rx else _time.time(),
                       "tweaks": self.tweaks, "decode_notes": self.decode_notes + self.tweaks}
            if self._rx is not None and self._rx.cfg.reports:
                message["report"] = self._report()
            if self.on_message is not None:
                self.on_message(message)
        self.decode_result = "stop"

    def _report(self):
        """The measured report of this decode (reports=True) through ft8rx_report_probe -- the batch's measurement step on this
        cycle's spectrum: the word is packed back from the text (the a-priori step keeps its own), None where that is not possible."""
        from . import synth
        rx, o = self._rx, self.origin
        word = getattr(self, "ap_result", None) and self.ap_result["word"]
        if not word:
            try:
                word = synth.pack77(*self.decode_result)
            except (ValueError, TypeError, IndexError, KeyError):
                return None
        spec = self._cycle_spectrum()
        with rx._hlock:
            rp = rx._handle(1).report_probe(spec[None], [0], [o["f0_idx"]], [o["h0_idx"]], [self._tt], [self._ft], [word])
        return _m.report_dict(rp[0])

    def _cycle_spectrum(self):
        """The cycle spectrum behind this candidate's grid: audio_in's, or -- a candidate of search(channel=j) -- that of channel j's
        frame of the newest complete cycle of its parity (wide_in.WideIn.cycle_spectrum)"""
        rx, o = self._rx, self.origin
        if "channel" in o:
            return rx.wide_in.cycle_spectrum(o["channel"], o["odd_even"])
        return rx.audio_in.get_cycle_spectrum()

    def _take_llr(self, llr, sd, snr, source):                       # the tail of _dB_to_llr (receiver.py:208-222)
        self.llr, self.llr_sd, self.snr, self.source = np.array(llr, np.float32), float(sd), int(snr), source
        if self.llr_sd <= self.llr_sd_min:
            self.decode_result = "stop"

    def _set_AP(self, k):                                            # receiver.py:109-117
        self.pat_name, b0, bits = AP_PATTERNS[k]
        self.llr = self.llr0.copy()
        for i, c in enumerate(bits):
            self.llr[b0 + i] = 5.0 if c == "1" else -5.0
        if self.pat_name == "CQ":
            self.llr[74:76] = -5.0
            self.llr[76] = 5.0
            self.llr[57:59] = -5.0

    def _attempt(self, what, args):                                  # _decode_good91 / _decode_ldpc / _decode_osd (receiver.py:119-135)
        from . import decoders as D
        if self.decode_result:
            return
        if what == "good91":
            self.decode_notes = f"{self.source}_{self.pat_name}_GOOD91 "
            self.decode_result = D.crc_unpack91(self.llr[:91])
        elif what == "ldpc":
            max_nc0, max_its, save = args
            self.decode_notes = f"{self.source}_{self.pat_name}_LDPC{max_its}"
            self.decode_result, self.n_its, out = D.ldpc_decode(self.llr, max_nc0, max_its)
            if save and not self.decode_result and len(out) == 174:
                self.saved_llrs.append((f"{self.pat_name}_LDPC{max_its}", out))
        else:
            self.decode_notes = f"{self.source}_{self.pat_name}_OSD"
            rx = self._rx
            if rx is not None and rx.cfg.weak:                       # weak mode: every trial within the distance gate (ft8rx_set_weak)
                with rx._hlock:
                    ok, lo, hi, _ = rx._handle(1).osd(np.asarray(self.llr, np.float32)[None], 30, 2, 0, _weak_osd_max_hd(rx.cfg))
                self.decode_result = D.unpack(D._msg(lo[0], hi[0])) if ok[0] else None
            else:
                self.decode_result = D.osd_012(self.llr)

    def _decode_ap_calls(self, rx):
        """ipass 7 (ft8rx_set_ap_calls) of this candidate through the single-vector entry points, as k_bp_ap / k_osd_ap /
        k_select_ap do it in the batch: every enabled pattern on the fine LLRs, the smallest distance within ap_max_hd wins.  The
        valid words met before the accepted one go through the call-hash table first, as the batch's replay of its events does."""
        from . import decoders as D
        from . import synth
        bits, mask = _lib.ap_patterns(rx.cfg.ap_my_call, rx.cfg.ap_dx_call)
        max_hd = rx.cfg.ap_max_hd if rx.cfg.ap_max_hd is not None else _lib.AP_MAX_HD_DEFAULT
        met = []
        with rx._hlock:
            best = ap_calls_attempts(rx._handle(1), rx.cfg, self.llr0, bits, mask, max_hd, rx._hlock, synth, met)
        if best is None:
            for _, w in met:
                D.unpack(w)
            return False
        ap, word, hd, method = best
        for a, w in met:
            if a < ap:
                D.unpack(w)
        self.decode_result = D.unpack(word)
        self.ap_result = dict(ap=ap, word=word, osd_hd=hd, method=method)
        self.decode_notes = "fine_" + _m.AP_CALL_NAMES[ap - 5].replace(" ", "_") + "_" + ("LDPC20", "OSD", "CODEWORD")[(2, 3, 5).index(method)]
        return self.decode_result is not None

    def decode(self, current_max_ipass):
        """One step of the ipass ladder per call (reference receiver.py:68-107)."""
        if self._rx is None:
            raise _lib.Ft8rxError("this Candidate is a plain record view; Receiver.search() returns decodable ones")
        if self.ipass > current_max_ipass or self.decode_result == "stop":
            return
        rx, o = self._rx, self.origin
        step = self.ipass
        if step == 0:
            with rx._hlock:
                llr, sd, snr = rx._handle(1).llr_grid(self._grid, [0], [o["f0_idx"]], [o["h0_idx"]])
            self._take_llr(llr[0], sd[0], snr[0], "grid")
            self.llr0 = self.llr.copy()
        elif step == 1:                                              # _get_llr_fine (receiver.py:140-173)
            spec = self._cycle_spectrum()
            with rx._hlock:                                          # weak mode: the joint three-block scan (ft8rx_fine_weak)
                f = rx._handle(1).fine(spec[None], [0], [o["f0_idx"]], [o["h0_idx"]], weak=rx.cfg.weak)
            tt, ft = int(f["ttweak"][0]), int(f["ftweak"][0])
            self.tweaks = " t:%+03d f:%+03d" % (tt, ft)
            self.n_sync_matches = int(f["nsync"][0])
            if self.n_sync_matches > 6:
                o.update({"tsec": float(o["tsec"] + tt / 200), "fHz": float(o["fHz"] + ft / 16)})
                self._tt, self._ft = tt, ft
                self._take_llr(f["llr"][0], f["sd"][0], f["snr"][0], "fine")
            else:
                self.source = "fine"
                self.decode_result = "stop"
        elif step == 6:
            for self.pat_name, self.llr in self.saved_llrs:
                self._attempt("osd", None)
        elif step == 7:
            found = False
            if self.source == "fine" and not self.decode_result and (rx.cfg.ap_my_call or rx.cfg.ap_dx_call):
                found = self._decode_ap_calls(rx)
            if not found:
                self.decode_result = "stop"
        if step == 2:
            self.llr0 = self.llr.copy()
        if step in _LADDER:
            what, variants, args = _LADDER[step]
            for k in variants:
                self._set_AP(k)
                if what == "good91+ldpc":
                    self._attempt("good91", None)
                    self._attempt("ldpc", args)
                else:
                    self._attempt(what, args)
        self.ipass += 1


def _pyaudio_device(audio_in, keywords):
    """True iff PyAudio is importable and a capture device matches `keywords` (sets audio_in.input_device_idx like the reference)."""
    try:
        import pyaudio
    except ImportError:
        return False
    try:
        return audio_in._find_input_device(keywords, pyaudio.PyAudio()) is not None
    except Exception:       # noqa: BLE001 -- no usable PortAudio host: behave like "no device"
        return False


def _as_frames(audio_i16):
    """[B, 180000] int16 as is; lists / short frames through frames_from_ragged."""
    if isinstance(audio_i16, np.ndarray) and audio_i16.dtype == np.int16 and audio_i16.ndim == 2 and audio_i16.shape[1] == _lib.NSAMP:
        return np.ascontiguousarray(audio_i16)
    if isinstance(audio_i16, np.ndarray) and audio_i16.ndim == 2:
        return frames_from_ragged(list(audio_i16))
    return frames_from_ragged(audio_i16)


def _as_frames_f32(audio):
    """The float flavour (float_frames=True): anything frames_from_ragged_f32 takes, [B, n] arrays included"""
    if isinstance(audio, np.ndarray) and audio.ndim == 2:
        return frames_from_ragged_f32(list(audio))
    return frames_from_ragged_f32(audio)


class AudioIn:
    """Host-side state the reference keeps per receiver (receiver.py:225-306): the 15-s audio ring, the
    750 x 976 search grid that the GUI's waterfall views in place, and the hop pointer.

    Two ways to fill it:
      * load_frame(audio)  -- frame-complete: one GPU spectrogram launch for all 375 hops;
      * _callback(in_data, frame_count, time_info, status_flags) -- streaming: the PortAudio
        callback signature of the reference (receiver.py:295-306).  Each call appends one 480-sample hop,
        advances search_grid_ptr exactly like the reference (wall-clock re-sync at the grid wrap) and writes
        that hop's 976 dB values, computed on the GPU (ft8rx_hop_spectrum), into search_grid[ptr] in place.
    Unlike the reference, decoding is triggered when a cycle's 375 hops are complete (Receiver.poll), not at
    hop 260 -- the frame-complete semantics of this build."""

    def __init__(self, search_freq_range, receiver, input_device_keywords=None):
        self.input_device_idx = None
        self.input_device_keywords = input_device_keywords
        self.stream = None
        self._feeder = None
        self.search_hps, self.search_bpt = 4, 2
        self.search_freq_range = search_freq_range
        self.search_fft_len = 3840
        self.samples_perhop = 480
        self.df = SYM_RATE / self.search_bpt
        self.search_f0_idx_range = [int(search_freq_range[0] / self.df), int(search_freq_range[1] / self.df)]
        self.search_hops_per_cycle = int(T_CYC * SYM_RATE * self.search_hps)
        self.search_hops_per_grid = 2 * self.search_hops_per_cycle
        self.dt = T_CYC / self.search_hops_per_cycle
        self.samples_per_cycle = SAMP_RATE * T_CYC
        # reference receiver.py:240: f0_hi + 8 * bpt columns (976 at the default range)
        self.search_grid = np.ones((self.search_hops_per_grid, self.search_f0_idx_range[1] + 8 * self.search_bpt), dtype=np.float32)
        self._rx = receiver
        self.search_grid_ptr = int(self._grid_time() * self.search_hops_per_grid / (2 * T_CYC))
        self.audio_buffer = np.zeros(self.samples_per_cycle, dtype=np.int16)    # reference: float32 copies of int16 samples
        self._audio = None
        self.cycle_spectrum = None
        self.cycles_completed = 0
        self._ready = []                 # (int16 frame, cycle start time) of completed, not yet decoded cycles
        self._lock = _threading.Lock()   # _callback may run on an audio thread, poll() on the manage_cycle stand-in
        d = WATERFALL_DOWNSAMPLE
        self.waterfall_data = {"data": self.search_grid[::d, ::d].T, "df": self.df * d, "dt": self.dt * d,
                               "sig_w": int(79 * self.search_hps / d), "sig_h": int(8 * self.search_bpt / d),
                               "pixels_per_cycle": int(self.search_hops_per_cycle / d)}

    def _grid_time(self):
        return self._rx.time_source() % (2 * T_CYC)

    # ---- audio sources (reference receiver.py:252-270)
    def _find_input_device(self, input_device_keywords, pya):
        """First PortAudio device whose name contains every comma-separated keyword (reference receiver.py:254-264)."""
        for dev_idx in range(pya.get_device_count()):
            name = pya.get_device_info_by_index(dev_idx)["name"]
            if all(pat in name for pat in input_device_keywords.replace(" ", "").split(",")):
                self.input_device_idx = dev_idx
                break
        return self.input_device_idx

    def open(self, source=None):
        """Start feeding _callback.
        source None : PortAudio capture through PyAudio (imported lazily; reference receiver.py:266-270): int16 mono 12 kHz,
                      480 frames per buffer, this object's _callback as the stream callback;
        otherwise   : any iterable of hops -- 480 int16 samples as an array or bytes -- consumed by a daemon thread that calls
                      _callback per hop.  Pacing is the iterator's business (a live source blocks until the next hop exists; a
                      file replayer sleeps; a test advances its virtual clock inside the generator)."""
        if source is None:
            try:
                import pyaudio
            except ImportError as e:
                raise _lib.Ft8rxError("AudioIn.open(): PyAudio is not installed -- pass an iterator of 480-sample int16 hops instead") from e
            pya = pyaudio.PyAudio()
            if self.input_device_idx is None and self.input_device_keywords:
                self._find_input_device(self.input_device_keywords, pya)
            self.stream = pya.open(format=pyaudio.paInt16, channels=1, rate=SAMP_RATE, input=True, input_device_index=self.input_device_idx,
                                   frames_per_buffer=self.samples_perhop, stream_callback=self._pa_callback)
            self.stream.start_stream()
            return self

        def feed():
            try:
                for hop in source:
                    if self._rx._stop.is_set():
                        break
                    self._callback(hop if isinstance(hop, (bytes, bytearray, memoryview)) else np.ascontiguousarray(hop, np.int16).tobytes(),
                                   self.samples_perhop, None, None)
                else:
                    self.source_exhausted = True
            except Exception as e:          # noqa: BLE001 -- surfaced by Receiver.poll()/stop() instead of dying silently on a daemon thread
                self._rx.thread_error = e
            finally:
                self._feeder = None         # a later start() opens a source again instead of running with no input
        self.source_exhausted = False
        t = self._feeder = _threading.Thread(target=feed, name="ft8rx-audio-in", daemon=True)
        t.start()
        return self

    def _pa_callback(self, in_data, frame_count, time_info, status_flags):
        import pyaudio
        self._callback(in_data, frame_count, time_info, status_flags)
        return (None, pyaudio.paContinue)

    def close(self, timeout=5.0):
        """Stop the PortAudio stream / wait for the feeder thread (which ends at its next hop once the receiver's stop flag is set)."""
        if self.stream is not None:
            try:
                self.stream.stop_stream()
                self.stream.close()
            finally:
                self.stream = None
        t = self._feeder
        if t is not None and t is not _threading.current_thread():
            t.join(timeout)
            if not t.is_alive():
                self._feeder = None

    def load_frame(self, audio_i16):
        """Frame-complete stand-in for 375 calls of _callback (receiver.py:295-306)."""
        self._audio = np.ascontiguousarray(audio_i16, np.int16).reshape(_lib.NSAMP)
        self.audio_buffer[:] = self._audio
        with self._rx._hlock:
            g = self._rx._handle(1).spectrogram(self._audio)[0]
        self.search_grid[1:376] = g[1:376, :self.search_grid.shape[1]]          # in place: waterfall_data['data'] is a live view
        self.search_grid_ptr = 375
        self.cycle_spectrum = None

    def _callback(self, in_data, frame_count=None, time_info=None, status_flags=None):
        samples = np.frombuffer(in_data, dtype=np.int16)
        n = len(samples)
        self.audio_buffer[:-n] = self.audio_buffer[n:]
        self.audio_buffer[-n:] = samples
        self.search_grid_ptr = (self.search_grid_ptr + 1) % self.search_hops_per_grid
        # a cycle is complete when the pointer reaches a multiple of 375 -- decided BEFORE the wall-clock re-sync below, which
        # moves the pointer away from 0 whenever the stream lags the clock (normal after PortAudio's start-up latency)
        cycle_done = self.search_grid_ptr % self.search_hops_per_cycle == 0
        if self.search_grid_ptr == 0:
            tg = self._grid_time()
            if tg > 0.1:
                self.search_grid_ptr = int(tg * self.search_hops_per_grid / (2 * T_CYC))
        # the live path has a handle of its own (Receiver._live): a hop arriving while the owner runs decode_frames / search on the
        # receiver's main handle must not touch that handle's staging audio, scratch rows or result slots
        with self._rx._live_lock:
            self.search_grid[self.search_grid_ptr, :] = self._rx._live_handle().hop_spectrum(self.audio_buffer[-self.search_fft_len:])[:self.search_grid.shape[1]]
        in_cycle = self.search_grid_ptr % self.search_hops_per_cycle
        if cycle_done:                                                   # the last hop of a cycle just landed
            self._audio = self.audio_buffer.copy()
            self.cycle_spectrum = None
            self.cycles_completed += 1
            with self._lock:
                self._ready.append((self._audio, self._rx.time_source(), 0))
        elif in_cycle in self._rx.early_decode_hops:
            # early pass (reference receiver.py:389-401 decodes candidates as their signals complete, first messages at ~12.9 s): the
            # cycle so far, silence after it -- the payload of every signal that started by +0.96 s has arrived at hop 320 (12.8 s), by
            # +1.76 s at hop 340 (13.6 s)
            part = np.zeros(_lib.NSAMP, np.int16)
            n_have = in_cycle * self.samples_perhop
            part[:n_have] = self.audio_buffer[-n_have:]
            with self._lock:
                self._ready.append((part, self._rx.time_source(), in_cycle))
        return (None, 0)                 # (None, pyaudio.paContinue)

    def get_cycle_spectrum(self):
        """First 49152 (wide build: 96000) bins of the reference's 96001-bin spectrum (receiver.py:280-286): all the fine sync reads."""
        if self.cycle_spectrum is None:
            if self._audio is None:
                raise _lib.Ft8rxError("no frame loaded")
            with self._rx._hlock:
                self.cycle_spectrum = self._rx._handle(1).cycle_spectrum(self._audio)[0]
        return self.cycle_spectrum


_FREQ_RANGE_DEFAULT = [100, 3000]                     # Receiver's defaults as objects: decode_frames_ft4 tells "not given" from them
_TIME_RANGE_DEFAULT = [-2.5 + 0.5, 2.5 + 0.5]


class Receiver:
    def __init__(self, input_device_keywords, on_message, sync_score_min=85, max_cands=200,
                 search_freq_range=_FREQ_RANGE_DEFAULT, search_time_range=_TIME_RANGE_DEFAULT, verbose=False,
                 device=0, max_frames=1, time_source=None, sleep=None, audio_source=None, autostart=None, early_decode_hop=(320, 340),
                 sample_rate=None, iq=False, dial_offsets_hz=(0.0,), bands=None, t_first=None, resample=False, waterfall=False,
                 modes=None, **extension_knobs):
        if search_freq_range[1] > 5900 or search_freq_range[0] < 12.5 or search_freq_range[0] >= search_freq_range[1]:
            # the reference sizes its grid from search_freq_range (receiver.py:234-240) and itself fails beyond ~5940 Hz, where the
            # fine-sync slice runs off the cycle spectrum (receiver.py:181-182).  Here the layouts are compile-time: up to 3000 Hz runs
            # on libft8rx.so, beyond that on libft8rx_wide.so (include/ft8rx.h), chosen by _lib.Handle from cfg.f0_hi
            raise _lib.Ft8rxError(f"search_freq_range {list(search_freq_range)} outside the supported [12.5, 5900] Hz")
        self.on_message = on_message
        self.time_source = time_source or _time.time          # the reference's time_utils seam (time_utils.py:7-8)
        self.sleep = sleep or _time.sleep                     # time_utils.py:13-14
        self._stop = _threading.Event()
        self._thread = None
        # Two handles, two locks.  The owner's calls (decode_frames, search, load_frame, get_cycle_spectrum) share the main handle
        # self._h under _hlock -- including its reallocation in _handle().  The live path (audio callback: hop spectra; manage_cycle
        # stand-in: poll) runs on its own one-frame handle self._live under _live_lock, so a hop that arrives in the middle of a
        # multi-pass decode cannot touch the main handle's staging audio, scratch rows or result slots.
        self._hlock = _threading.RLock()
        self._live_lock = _threading.RLock()
        self._live = None
        self.thread_error = None
        # streaming: also decode the partial cycle when these hops have arrived (320 = 12.8 s, 340 = 13.6 s into the cycle), so that
        # most messages are delivered before the next cycle starts, as the reference's are (its first decodes appear at ~12.9 s,
        # tests/PyFT8.txt:1-19); one hop, a sequence of hops, or None / 0 / () = only at the end of the cycle
        if isinstance(early_decode_hop, str):
            # "incremental": the reference starts on each candidate as soon as its payload has arrived (manage_cycle polls every 0.1 s from
            # hop 260, receiver.py:389-401); here the partial cycle is decoded every 5 hops (0.2 s) from hop 300 -- the payload of a signal
            # that starts at 0 s is complete at hop 296 -- so every message is delivered within 0.2 s of its last payload symbol
            if early_decode_hop != "incremental":
                raise _lib.Ft8rxError('early_decode_hop: a hop, a sequence of hops, None or "incremental"')
            early_decode_hop = tuple(range(300, 375, 5))
        if isinstance(early_decode_hop, range):
            early_decode_hop = tuple(early_decode_hop)
        hops = early_decode_hop if isinstance(early_decode_hop, (tuple, list)) else ((early_decode_hop,) if early_decode_hop else ())
        hops = tuple(sorted({int(x) for x in hops}))
        if any(not 300 <= x < 375 for x in hops):
            raise _lib.Ft8rxError("early_decode_hop: hops must lie in [300, 375) (the payload of a signal that starts at 0 s is complete at hop 296) or be None")
        self.early_decode_hops = hops
        self.early_decode_hop = hops[-1] if hops else None    # the last early pass
        self._cycle_seen = {}                                 # cycle start -> message texts already delivered (early pass, then the full one)
        self.sync_score_min, self.max_cands = sync_score_min, max_cands
        self.verbose = verbose
        self.band = None
        self.candidates = []
        # recall (ipass 8): poll feeds each complete cycle the messages of the cycle 30 s before it
        self.recall = bool(extension_knobs.pop("recall", False))
        # measured reports: every message dict gains "report", the measured SNR / frequency / start time
        self.reports = bool(extension_knobs.pop("reports", False))
        self._recall_hist = {}                                # cycle start -> complete-frame message dicts (recall = True)
        # noise blanker: None / False = off, True = the defaults, a number = the threshold k, a dict of threshold /
        # guard / taper.  An input stage, not a handle setting: the frames are blanked on the GPU (ft8rx_blank) wherever they are about
        # to be decoded -- decode_frames / decode_frames_arrays (once, before the first pass), decode_stream (behind the
        # down-converter), the live passes of poll (early passes included) -- and everything behind sees ordinary frames.  The live
        # search_grid / waterfall of audio_in, and search() on it, stay the unblanked audio.  blanker_stats: the last batch's int32
        # [B, 4] = hits, samples with w < 32768, samples with w = 0, blocks with L_b = 0 per frame.
        self.noise_blanker = _blanker.params(extension_knobs.pop("noise_blanker", None))
        self.blanker_stats = None
        # float frames: the default of float_frames= of decode_frames / decode_frames_arrays / decode_frame /
        # decode_stream, and what the wide live input runs
        self.float_frames = bool(extension_knobs.pop("float_frames", False))
        refuse_float_with_blanker(self.float_frames, self.noise_blanker)
        # input blanker: the same values, and a dict may also hold block.  An input stage in FRONT of the
        # down-converter: ONE stream of integer samples is blanked at its own rate on the GPU (ft8rx_blank_in*) and handed to the
        # front end on the device -- decode_stream (its own keyword overrides this one) and the wide live input.  Unlike noise_blanker
        # the live search grid / waterfall of the channels show the blanked input.  input_blanker_stats: the cumulative int64 [4].
        self.input_blanker = extension_knobs.pop("input_blanker", None)
        _wide_in.input_blanker_params(self.input_blanker, 17, 1, 240000)      # a value outside the definition is refused here
        self._input_blanker_stats = None
        # panorama: None / True / a dict of n_fft, n_avg or period_s, rows.  An input stage beside the down-
        # converter: the averaged power spectrum and rail count of ONE raw stream at its own rate (ft8rx_pan*) -- decode_stream (its own
        # keyword overrides this one) and the wide live input.  `panorama` holds the result.
        self.panorama_opt = extension_knobs.pop("panorama", None)
        _pan.params(self.panorama_opt, 240000)                                # a value outside the definition is refused here
        self._panorama = None
        # FT4 (decode_frames_ft4): its knobs (None = the library's defaults) and its search range -- the
        # ranges given here, or FT4's own defaults (12.5 .. 5900 Hz, starts -0.5 .. +2.0 s) where the FT8 defaults were left alone
        self.ft4_sync_min = extension_knobs.pop("ft4_sync_min", None)
        self.ft4_osd_max_hd = extension_knobs.pop("ft4_osd_max_hd", None)
        # ft4_passes (section 19.6): 1 = one pass; 2, 3 = remove the decoded signals and decode the residual again, that often.
        # ft4_sub_osd_max_hd: OSD's distance gate in the passes after the first (None = the first pass's gate)
        self.ft4_passes = extension_knobs.pop("ft4_passes", 1)
        if isinstance(self.ft4_passes, bool) or not isinstance(self.ft4_passes, (int, np.integer)) or not 1 <= self.ft4_passes <= 3:
            raise _lib.Ft8rxError(f"ft4_passes must be 1, 2 or 3, got {self.ft4_passes!r}")
        self.ft4_passes = int(self.ft4_passes)
        self.ft4_sub_osd_max_hd = extension_knobs.pop("ft4_sub_osd_max_hd", None)
        # ft4_coherent (section 19.8): the candidates BP leaves undecoded are decoded again on LLRs over runs of two and four symbols,
        # before OSD; every FT4 message dict then says "nsym": 1, 2 or 4.  Applied in _ft4_set, so every FT4 pass gets it.
        self.ft4_coherent = extension_knobs.pop("ft4_coherent", False)
        if not isinstance(self.ft4_coherent, (bool, np.bool_)):
            raise _lib.Ft8rxError(f"ft4_coherent must be True or False, got {self.ft4_coherent!r}")
        self.ft4_coherent = bool(self.ft4_coherent)
        # ft4_weak (section 19.10): the search is the coherent Costas sync on the 2.6-Hz grid, cut at ft4_weak_min (None = the library's
        # default) instead of ft4_sync_min; everything behind the candidate list is as before.  Applied in _ft4_set.
        self.ft4_weak = extension_knobs.pop("ft4_weak", False)
        if not isinstance(self.ft4_weak, (bool, np.bool_)):
            raise _lib.Ft8rxError(f"ft4_weak must be True or False, got {self.ft4_weak!r}")
        self.ft4_weak = bool(self.ft4_weak)
        self.ft4_weak_min = extension_knobs.pop("ft4_weak_min", None)
        # ft4_coh_osd (section 19.11): behind the coherent step and OSD, OSD runs once more on the run-of-2 and run-of-4 rows, and a
        # word it returns is taken where its whole-message score reaches ft4_coh_osd_min_score (None = the library's default).  It
        # acts on the coherent rows, so it needs ft4_coherent=True.  Applied in _ft4_set.
        self.ft4_coh_osd = extension_knobs.pop("ft4_coh_osd", False)
        if not isinstance(self.ft4_coh_osd, (bool, np.bool_)):
            raise _lib.Ft8rxError(f"ft4_coh_osd must be True or False, got {self.ft4_coh_osd!r}")
        self.ft4_coh_osd = bool(self.ft4_coh_osd)
        self.ft4_coh_osd_min_score = extension_knobs.pop("ft4_coh_osd_min_score", None)
        if self.ft4_coh_osd and not self.ft4_coherent:
            raise _lib.Ft8rxError("ft4_coh_osd=True needs ft4_coherent=True: it runs OSD on the coherent step's LLRs")
        # ft4_reports (section 19.9): every FT4 message is measured against its own model on the audio its pass decoded (SNR,
        # frequency, start time) and its dict gains "report".  An FT4 knob of the receiver, not a row of the opt-in table.
        self.ft4_reports = extension_knobs.pop("ft4_reports", False)
        if not isinstance(self.ft4_reports, (bool, np.bool_)):
            raise _lib.Ft8rxError(f"ft4_reports must be True or False, got {self.ft4_reports!r}")
        self.ft4_reports = bool(self.ft4_reports)
        # live FT4 (section 19.7; modes= here or in start()): the early passes of a 7.5-s slot, seconds into it -- one at 6.0 s (72000
        # samples) by default, () = only the complete slot
        self.ft4_early_samples = _wide_in.ft4_early_samples(extension_knobs.pop("ft4_early_decode_s", _wide_in.FT4_EARLY_S_DEFAULT))
        self._ft4_freq_range = None if search_freq_range is _FREQ_RANGE_DEFAULT else tuple(search_freq_range)
        self._ft4_time_range = None if search_time_range is _TIME_RANGE_DEFAULT else tuple(search_time_range)
        self.cfg = config_from_kwargs(sync_score_min, max_cands, search_freq_range, search_time_range, **extension_knobs)
        if self.recall:
            _optins.refuse(_optins.RECALL, _optins.active(self.cfg))
        self.cfg.recall = self.recall
        self.cfg.reports = self.reports
        self.search_h0_range = [self.cfg.h0_lo, self.cfg.h0_hi]
        self.search_start_hop = self.search_h0_range[1] + 43 * 4
        self.device = device
        self._h = None
        self.subtract_refine = 2              # multi-pass decode: how origins are re-estimated before subtraction (_lib.Handle.subtract):
                                              # 2 = on a decimated baseband copy (same yield as the full-rate scans of 1, 5x faster)
        self.call_hashes = _lib.CallHashTable()       # persistent across the cycles of the stream (poll); batches use fresh ones
        self._handle(max_frames)                      # fail loudly now if there is no GPU / library
        self.audio_in = AudioIn(search_freq_range, self, input_device_keywords)
        # wide live input (sample_rate given): the source delivers real or IQ chunks at 12 .. 192 kHz, which
        # the streaming down-converter turns into the channels dial_offsets_hz on the live handle (wide_in.WideIn; wide_in.push(chunk)
        # may also be called directly).  audio_in stays the 12 kHz object; with waterfall=True the channels have a search grid and a
        # waterfall of their own (wide_in.search_grid[j] / .waterfall_data[j], search(channel=j)).
        self.wide_in = None
        self._set_wide_in(sample_rate, iq, dial_offsets_hz, bands, t_first, resample, waterfall, modes)
        # The reference starts its audio thread and manage_cycle in the constructor (receiver.py:252, 336).  Same here when there
        # is something to listen to: an explicit audio_source, or PortAudio (PyAudio importable and a device matches the keywords).
        if autostart is None:
            autostart = audio_source is not None or (bool(input_device_keywords) and _pyaudio_device(self.audio_in, input_device_keywords))
        if autostart:
            self.start(audio_source)

    def _set_wide_in(self, sample_rate, iq, dial_offsets_hz, bands, t_first, resample, waterfall=False, modes=None):
        """The wide live input of the constructor's and start()'s arguments; sample_rate None leaves what there is.  modes (DESIGN.md
        section 19.7): per-channel "FT8" / "FT4"; with an FT4 channel the opt-ins FT4 does not run with are refused here, before a stream
        opens"""
        if sample_rate is None:
            if modes is not None:
                raise _lib.Ft8rxError("modes: per-channel modes belong to the wide live input (sample_rate=, dial_offsets_hz=)")
            return
        if _wide_in.channel_modes(modes, len(dial_offsets_hz)) is not None:
            self._refuse_with_ft4_channels()
        self.wide_in = _wide_in.WideIn(self, sample_rate, iq=iq, dial_offsets_hz=dial_offsets_hz, bands=bands, t_first=t_first, resample=resample,
                                       waterfall=waterfall, input_blanker=self.input_blanker, float_frames=self.float_frames,
                                       **({"panorama": self.panorama_opt} if self.panorama_opt else {}),
                                       **({"modes": modes} if modes is not None else {}))

    def _refuse_with_ft4_channels(self):
        """An FT4 channel of the live stream (modes=) and what FT4 does not run with: the rows of the opt-in table (optins.FT4: my_call /
        dx_call, recall, weak, reports), and the two frame stages FT4 has no form of"""
        _optins.refuse(_optins.FT4, _optins.active(self.cfg, recall=self.recall))
        name = _optins.TABLE[_optins.FT4][0]
        if self.noise_blanker is not None:
            raise _lib.Ft8rxError(f"{name} is not supported together with noise_blanker: it blanks 15-s frames")
        if self.float_frames:
            raise _lib.Ft8rxError(f"{name} is not supported together with float_frames=True: FT4 frames are int16")

    @property
    def panorama(self):
        """The panorama: the live stream's dict (wide_in.panorama), else the last decode_stream's; None while off"""
        live = self.wide_in.panorama if self.wide_in is not None else None
        return live if live is not None else self._panorama

    @property
    def input_blanker_stats(self):
        """int64 [4] of the input blanker: the live stream's cumulative counts, else the last decode_stream's; None while it is off"""
        live = self.wide_in.input_blanker_stats() if self.wide_in is not None else None
        return live if live is not None else self._input_blanker_stats

    # ---- the manage_cycle stand-in (reference receiver.py:336, 372-412)
    def start(self, audio_source=None, sample_rate=None, iq=False, dial_offsets_hz=(0.0,), bands=None, t_first=None, resample=False,
              waterfall=False, modes=None):
        """Open the audio source (AudioIn.open) and start the daemon that decodes completed cycles: every 0.1 s (the reference's
        poll period, receiver.py:383) it calls poll(); on_message runs on that thread, as in the reference.  Unlike the
        reference, whose daemon dies on the first exception, an exception is kept in .thread_error and the loop ends.
        sample_rate (here or in the constructor): audio_source is an iterator of chunks of any length at that rate -- real, or IQ
        with iq=True, the forms of decode_stream -- feeding the channels dial_offsets_hz (wide_in.WideIn.open); t_first = the time of
        its first sample (default: time_source() at the first chunk).  resample=True: a rate that is no multiple of 12 kHz goes through
        the rational resampler (wide_in.WideIn).  waterfall=True: the channels' search grids and waterfalls are
        kept (wide_in.WideIn, section 16.5).  modes: "FT8" / "FT4" for every channel or one per channel (section 19.7)."""
        if self._thread is not None and self._thread.is_alive():
            return self
        self._stop.clear()
        self.thread_error = None
        self._set_wide_in(sample_rate, iq, dial_offsets_hz, bands, t_first, resample, waterfall, modes)
        if self.wide_in is not None:
            if audio_source is not None:
                self.wide_in.open(audio_source)
        else:
            if self.audio_in._feeder is not None and not self.audio_in._feeder.is_alive():
                self.audio_in._feeder = None
            if audio_source is not None or self.audio_in.stream is None and self.audio_in._feeder is None:
                self.audio_in.open(audio_source)

        def manage_cycle():
            try:
                while not self._stop.is_set():
                    self.sleep(0.1)
                    self.poll()
            except Exception as e:              # noqa: BLE001 -- surfaced to the owner instead of silently killing the daemon
                self.thread_error = e
        self._thread = _threading.Thread(target=manage_cycle, name="ft8rx-manage-cycle", daemon=True)
        self._thread.start()
        return self

    def stop(self, timeout=5.0):
        """Stop the daemon and the audio source, wait for both; an exception that ended either thread is raised here."""
        self._stop.set()
        if self._thread is not None and self._thread is not _threading.current_thread():
            self._thread.join(timeout)
        self.audio_in.close(timeout)
        if self.wide_in is not None:
            self.wide_in.close(timeout)
        self.close()
        self._raise_thread_error()

    def close(self):
        """Release the GPU handles (workspaces, page-locked buffers) of the batch and the live path; a later decode_frames / poll /
        search re-creates what it needs.  stop() calls this."""
        with self._hlock:
            if self._h is not None:
                self._h.close()
                self._h = None
        with self._live_lock:
            if self._live is not None:
                self._live.close()
                self._live = None

    def _raise_thread_error(self):
        e, self.thread_error = self.thread_error, None
        if e is not None:
            raise _lib.Ft8rxError(f"receiver thread failed: {type(e).__name__}: {e}") from e

    def _handle(self, n_frames):
        with self._hlock:
            if self._h is None or self._h.max_frames < n_frames:
                if self._h is not None:
                    self._h.close()
                self._h = _lib.Handle(self.cfg, device=self.device, max_frames=n_frames)
            # small batches: latency over work -- see ft8rx_set_ladder_mode
            self._h.set_ladder_mode(1 if n_frames < 128 else 0)       # crossover measured at 64..128 frames per call (profiles/archive/r02_latency.txt)
            return self._h

    def _live_handle(self, n_frames=1):
        """The live path's own handle (hop spectra and the per-cycle decodes of poll: one frame; wide input: one frame per channel,
        and the down-converter's stream); call with _live_lock held."""
        if self._live is None or self._live.max_frames < n_frames:
            if self._live is not None:
                self._live.close()
            self._live = _lib.Handle(self.cfg, device=self.device, max_frames=n_frames)
            self._live.set_ladder_mode(1)
        return self._live

    def set_band(self, band):
        self.band = band

    def _ap_on(self):
        return bool(self.cfg.ap_my_call or self.cfg.ap_dx_call)

    def set_ap_calls(self, my_call=None, dx_call=None):
        """The operator's own call and the call of the station being worked, as known bits of an extra decode step (ipass 7, after the
        reference's ladder).  None / "" = unset.  Cheap: call it whenever the DX station changes; in live mode it
        takes effect at the next cycle.  Standard callsigns only."""
        set_ap_calls_cfg(self.cfg, my_call, dx_call)
        with self._hlock:
            if self._h is not None:
                self._h.set_ap_calls(self.cfg.ap_my_call, self.cfg.ap_dx_call)
        with self._live_lock:
            if self._live is not None:
                self._live.set_ap_calls(self.cfg.ap_my_call, self.cfg.ap_dx_call)

    def _search_source(self, channel):
        """(the 750-row grid search() reads, the band of its candidates): audio_in's, or channel j's of the wide input"""
        if channel is None:
            return self.audio_in.search_grid, self.band
        w = self.wide_in
        if w is None or not w.waterfall:
            raise _lib.Ft8rxError(f"search(channel={channel}): the receiver keeps no grid of its channels (Receiver(..., sample_rate=, waterfall=True))")
        if not isinstance(channel, (int, np.integer)) or not 0 <= channel < w.n_channels:
            raise _lib.Ft8rxError(f"search(channel={channel}): the wide input has channels 0 .. {w.n_channels - 1}")
        if w.modes is not None and w.modes[channel] == _wide_in.FT4:
            raise _lib.Ft8rxError(f"search(channel={channel}): channel {channel} is an FT4 channel -- search() is FT8's Costas search")
        return w.search_grid[channel], (w.bands[channel] if w.bands is not None else self.band)

    def search(self, cyclestart_string, odd_even, search_f_idxs=None, channel=None):
        """Costas sync search over one cycle of audio_in.search_grid (reference receiver.py:338-367) -- or, with channel=j, of
        wide_in.search_grid[j] (waterfall=True): the candidates then carry band = bands[j] and "channel": j in
        their origin, and decode() on them takes the cycle spectrum of that channel's frame out of the down-converter's ring.

        odd_even selects the half of the 750-row grid (rows odd_even*375 + 1 ... + 375); hops before the cycle's
        first row read 1.0 (frame-complete semantics, DESIGN.md section 1 -- the live reference would see the
        tail of the previous cycle there).  search_f_idxs: any sequence of f0 indices (the reference iterates over it, keeps
        the f0 whose best score clears the threshold, sorts by score -- stably, so ties keep the iteration order -- and cuts
        at max_cands).  The configured range runs entirely on the device (k_sync + k_topk, as in the decode pipeline); any other
        sequence is one pass of the correlation kernel over [min, max] of the list on the same handle (ft8rx_sync_scores) followed
        by those three steps on the host."""
        if odd_even not in (0, 1):
            raise _lib.Ft8rxError("odd_even must be 0 or 1")
        search_grid, band = self._search_source(channel)
        if search_f_idxs is None:
            idx = list(range(*self.audio_in.search_f0_idx_range))
        else:
            idx = [int(i) for i in search_f_idxs]
        if not idx:
            self.candidates = []
            return []
        width = search_grid.shape[1]
        if min(idx) < 4 or max(idx) + 16 > width:
            raise _lib.Ft8rxError(f"search_f_idxs must stay within [4, {width - 16}] (the grid has {width} columns, receiver.py:240)")
        if len(set(idx)) != len(idx):
            raise _lib.Ft8rxError("search_f_idxs holds an index twice")
        r0 = odd_even * self.audio_in.search_hops_per_cycle
        rows = search_grid[r0 + 1:r0 + 376] if odd_even == 0 else np.concatenate([search_grid[r0 + 1:], search_grid[:1]])
        with self._hlock:
            h = self._handle(1)
            grid = np.ones((1, _lib.GRID_ROWS, h.grid_cols), np.float32)
            grid[0, 1:376, :width] = rows
            if self.cfg.weak:
                # weak mode: the three-block score (ft8rx_sync_scores_weak, k_sync3) over [min, max] of the list, then k_topk's steps
                # on the host with the weak threshold -- keep above it in iteration order, sort by score stably, cut at max_cands
                lo, hi = min(idx), max(idx) + 1
                sc, h0 = h.sync_scores(grid, lo, hi, weak=True)
                thr = np.float32(_lib.WEAK_SYNC_MIN_DEFAULT if self.cfg.weak_sync_min is None else self.cfg.weak_sync_min)
                found = [(f, int(h0[0, f - lo]), float(sc[0, f - lo])) for f in idx if sc[0, f - lo] > thr]
                found.sort(key=lambda c: -c[2])
                found = found[:self.cfg.max_cands]
            elif idx == list(range(*self.audio_in.search_f0_idx_range)):
                # the configured range: threshold / stable sort / cut on the device (k_topk), as in the decode pipeline
                f0, h0, sc, cnt = h.sync_search(grid)
                found = [(int(f0[0, i]), int(h0[0, i]), float(sc[0, i])) for i in range(int(cnt[0]))]
            else:
                # any other index sequence: ONE pass of the same correlation kernel over [min, max] on this handle
                # (ft8rx_sync_scores), then the reference's own steps on the host -- keep the f0 whose best score clears the
                # threshold, in iteration order; sort by score, stably; cut at max_cands (receiver.py:350-367)
                lo, hi = min(idx), max(idx) + 1
                sc, h0 = h.sync_scores(grid, lo, hi)
                thr = np.float32(self.cfg.sync_score_min)
                found = [(f, int(h0[0, f - lo]), float(sc[0, f - lo])) for f in idx if sc[0, f - lo] > thr]
                found.sort(key=lambda c: -c[2])
                found = found[:self.cfg.max_cands]
        cands = []
        for f0i, h0i, sci in found:
            origin = {"h0_idx": h0i, "f0_idx": f0i, "tsec": h0i / 25.0, "fHz": 3.125 * f0i, "score": sci,
                      "cyclestart_string": cyclestart_string, "band": band, "odd_even": odd_even}
            if channel is not None:
                origin["channel"] = int(channel)
            cands.append(Candidate(origin, [r0 + h0i + 4, r0 + h0i + 4 * 71], rx=self, grid=grid,
                                   llr_sd_min=-np.inf if self.cfg.weak else 5))      # weak mode: no sd stop at grid or fine
        self.candidates = cands
        return cands

    def decode_frames(self, audio_i16, cyclestart_strings=None, return_records=False, passes=1, subtract_min_snr=-10,
                      sub_pass_osd=True, research="full", recall=None, float_frames=None):
        """Decode B independent 15-s frames.  -> list (per frame) of message dicts in emit order.

        passes > 1 (extension): after each pass every newly decoded signal with SNR > subtract_min_snr is
        re-encoded and subtracted from the frame on the GPU (ft8rx_subtract -- the arithmetic of the reference experiment's
        Receiver.subtract_signal, tests/pipeline/receiver_sub.py:380-402, threshold :434) and the residual is decoded again;
        messages found that way are appended with "_SUB" added to decode_notes (as the reference tags them, :131-132).  Unlike
        the reference experiment -- which subtracts after every single decode, serially -- a pass subtracts all of a frame's
        new decodes at once, so whole batches stay on the GPU.  sub_pass_osd=False drops OSD decodes (ipass 5/6: first CRC-valid
        trial wins, the reference's source of false decodes) found in the later passes -- fewer false decodes, slightly less yield.
        research="local" is the experiment's re-search (receiver_sub.py:434-445), batched: the residual is searched only in the columns
        f0 - 2 .. f0 + 1 of the subtracted signals, with the sync threshold ignored (ft8rx_set_search_mask), and what that finds is not
        subtracted again -- one sweep for all of a frame's decodes where the experiment does one per decode.
        recall (ipass 8): per frame a list of the message dicts decoded 30 s before it in the same stream (or
        None / [] for none) -- their continuations are tested at the same positions; recall messages follow a frame's others and
        every dict gains "recall".  Of each frame's list the RECALL_MAX qualifying messages with the highest SNR are used.
        float_frames=True (default: the receiver's): the frames are float32 / float64 arrays (frames_from_ragged_f32)
        at any level and are decoded unrounded; the later passes subtract in float32 and do not round the residual."""
        f32 = self._float_frames(float_frames)
        audio = _as_frames_f32(audio_i16) if f32 else _as_frames(audio_i16)
        B = audio.shape[0]
        if B == 0:
            return ([], np.zeros((0, self.cfg.max_cands), _lib.RECORD_DTYPE), np.zeros(0, np.int32)) if return_records else []
        if recall is not None and len(recall) != B:
            raise _lib.Ft8rxError(f"recall: one list of earlier messages per frame ({B}), got {len(recall)}")
        with self._hlock:
            return self._decode_frames_locked(audio, B, cyclestart_strings, return_records, passes, subtract_min_snr, sub_pass_osd, research,
                                              recall, f32=f32)

    def _float_frames(self, float_frames):
        """float_frames= of an entry (None = the receiver's) -> bool; refused together with noise_blanker"""
        f32 = self.float_frames if float_frames is None else bool(float_frames)
        refuse_float_with_blanker(f32, self.noise_blanker)
        return f32

    def _local_mask(self, msgs, mcnt, min_snr):
        """Search mask of the local re-search: columns f0 - 2 .. f0 + 1 (receiver_sub.py:440) of every message the sweep subtracts."""
        B = len(mcnt)
        lo, hi = self.cfg.f0_lo, self.cfg.f0_hi
        mask = np.zeros((B, hi - lo), np.uint8)
        sel = (np.arange(msgs.shape[1])[None, :] < np.asarray(mcnt)[:, None]) & (msgs["snr"] > min_snr)
        fi, mi = np.nonzero(sel)
        f0 = msgs["f0_idx"][fi, mi].astype(np.int64)
        for d in (-2, -1, 0, 1):
            c = f0 + d
            ok = (c >= lo) & (c < hi)
            mask[fi[ok], c[ok] - lo] = 1
        return mask

    def _pass(self, h, B, frames, recall, gather=None, f32=False):
        """One decode of a batch of B frames on handle h, for every entry of this class; the caller holds h's lock.  frames: host frames
        int16 [B, 180000], or None = they are in h's staging buffer already (decode_stream), or `gather(h)` brings them there (the live
        wide input).  recall: the entries per frame (_recall_entries), or None = no recall step.  The noise blanker, when on, blanks the
        frames in the staging buffer first and leaves its counters in blanker_stats.  f32: the frames are float32 --
        host frames float32 [B, 180000], or in h's float staging buffer; the noise blanker is off then (refuse_float_with_blanker).
        -> (records, counts, events, event counts), (recall records, counts) or None, reports [B, max_cands] or None.
        A step around the decode of a batch belongs here ("Adding a step around the batch")."""
        if recall is not None:
            h.set_recall(recall)
        if gather is not None:
            gather(h)
        if f32:
            if frames is not None:
                res = h.decode_batch_f32(frames)
            else:
                h.enqueue_f32(h.staging_ptr_f32(), B)
                res = h.fetch(B)
        elif frames is not None and self.noise_blanker is None:
            res = h.decode_batch(frames)
        else:
            if self.noise_blanker is not None:
                self.blanker_stats = h.blank(None, B, *self.noise_blanker) if frames is None else h.blank_host(frames, *self.noise_blanker)
            h.enqueue(h.staging_ptr(), B)
            res = h.fetch(B)
        return res, (h.fetch_recall(B) if recall is not None else None), (h.fetch_reports(B) if self.reports else None)

    def _package(self, res, rres=None, **kw):
        """The native host message layer (multithreaded; messages.package_frame is its Python twin) for the results of _pass:
        ft8rx_package_batch_recall when the pass had a recall step, ft8rx_package_batch_ext when the config opts into more message
        types (msg_types != 0; rows of _lib.MESSAGE_EXT_DTYPE), else ft8rx_package_batch.  kw: table= / n_threads= of those."""
        if rres is not None:
            return _lib.package_batch_recall(*res, *rres, **kw)
        if self.cfg.msg_types:
            return _lib.package_batch_ext(*res, self.cfg.msg_types, **kw)
        return _lib.package_batch(*res, **kw)

    def _later_passes(self, h, B, passes, msgs, mcnt, res, min_snr, local, merge, f32=False, **pkg_kw):
        """Passes 2 .. `passes` of a batch whose frames pass 1 left in h's staging buffer (msgs, mcnt: its messages, res: its results):
        subtract the fresh messages of the pass before, decode the residual -- local: the experiment's local re-search, one sweep --
        and hand the packaged messages to merge(p, msgs, counts) -> the fresh ones (rows, counts).  -> the results of the last pass run.
        f32: the frames are in the float staging buffer and stay float32 between the passes (ft8rx_subtract_f32: no rounding)"""
        staging, enqueue = (h.staging_ptr_f32, h.enqueue_f32) if f32 else (h.staging_ptr, h.enqueue)
        for p in range(1, int(passes)):
            sigs = self._subtraction_list(msgs, mcnt, res[0], min_snr)
            if not sigs[1].any():
                break
            # the pass before left the frames in the handle's device buffer (f32: the float one, and the float entry)
            h.subtract(staging(), B, sigs, refine=self.subtract_refine, **({"float_frames": True} if f32 else {}))
            if local:
                h.set_search_mask(self._local_mask(msgs, mcnt, min_snr))
            try:
                enqueue(staging(), B)
                res = h.fetch(B)
            finally:
                if local:
                    h.set_search_mask(None)
            msgs, mcnt = merge(p, *_lib.package_batch(*res, **pkg_kw))
            if local:
                break                                                # candidates of the local re-search are not subtracted again (:444)
        return res

    def _recall_entries(self, recall):
        from . import recall as R
        return [R.entries_from_dicts(d or [], self.cfg) for d in recall]

    def decode_stream(self, samples, sample_rate, iq=False, dial_offsets_hz=(0.0,), src=None, bands=None, resample=False, **kw):
        """Decode one cycle of wider input: `samples` [n_streams][n] (one stream may come as [n]) at sample_rate = 12, 24, 48, 96 or
        192 kHz (or ONE stream at a wide rate, see below) -- real (sound card: int16 or float), or with iq=True complex baseband (SDR: complex, or int16 (I, Q) pairs
        [n_streams, n, 2]) -- is down-converted on the GPU (ft8rx_ddc) into one 12 kHz USB frame per entry of
        dial_offsets_hz: channel j is stream src[j] (default: stream 0, or stream j when there are as many streams as channels)
        with its dial dial_offsets_hz[j] Hz from the stream's centre (0 Hz for real input).  The frames never leave the device.
        -> list (per channel) of message dicts, exactly what decode_frames returns for those frames; its keyword arguments (passes,
        recall, cyclestart_strings, ...) work unchanged.  bands[j], when given, is the "band" of channel j's dicts; fHz stays the audio
        frequency inside the channel.
        A wide rate (a multiple of 48 kHz from 240 kHz to 129.6 MHz: ddc_wide.plan) takes ONE stream through the pre-decimator
        (ft8rx_ddc_wide); its kind is the dtype's: with iq=True uint8 (RTL-SDR), int8 (HackRF) or int16 (I, Q)
        pairs [n, 2], without it real int16 [n] (direct sampling; the dials are then absolute frequencies).  Float or complex samples
        are refused there.
        resample=True: the path is chosen by the rate -- a rate of ddc.RATES and a wide rate as above, any other rate that
        ddc_rat.accepts (44.1 kHz, 2.048 MS/s, 10 MS/s: ONE stream, any of the dtypes above) through the rational resampler
        (ft8rx_ddc_rat); a rate none of the three takes is refused, naming the rate.  Without it every rate
        behaves and is refused as it always was.
        input_blanker= (default: the receiver's; None / True / a threshold k / a dict of threshold, guard, taper, block): ONE stream
        of integer samples is blanked at its own rate on the device (ft8rx_blank_in_host) and the front end
        reads it there; more streams, or float / complex samples, are refused.
        float_frames= (default: the receiver's): the down-converter's output before rounding is decoded as float32
        frames -- a quiet wide source whose 12 kHz channels stay under one count of int16 decodes as at full level."""
        input_blanker = kw.pop("input_blanker", self.input_blanker)
        pn = _pan.params(kw.pop("panorama", self.panorama_opt), int(sample_rate))
        f32 = self._float_frames(kw.pop("float_frames", None))
        dials = [float(f) for f in dial_offsets_hz]
        n_out = len(dials)
        if n_out < 1:
            raise _lib.Ft8rxError("dial_offsets_hz: at least one channel")
        mod = _wide_in.front_end(sample_rate, resample)
        arr, kind, n_streams, _ = _wide_in.pack(samples, iq, sample_rate, mod)
        src = _wide_in.sources(mod, src, n_streams, n_out)
        if bands is not None and len(bands) != n_out:
            raise _lib.Ft8rxError(f"bands: one per channel ({n_out}), got {len(bands)}")
        if kw.get("recall") is not None and len(kw["recall"]) != n_out:
            raise _lib.Ft8rxError(f"recall: one list of earlier messages per channel ({n_out}), got {len(kw['recall'])}")
        args = {"cyclestart_strings": None, "return_records": False, "passes": 1, "subtract_min_snr": -10, "sub_pass_osd": True,
                "research": "full", "recall": None}
        for k in kw:
            if k not in args:
                raise TypeError(f"decode_stream() got an unexpected keyword argument '{k}'")
        args.update(kw)
        ib = _wide_in.input_blanker_params(input_blanker, kind, n_streams, int(sample_rate))
        if pn is not None:
            _pan.one_stream(True, n_streams)
        with self._hlock:
            h = self._handle(n_out)
            d_f32 = h.staging_ptr_f32() if f32 else None       # float frames: the audio before rounding, into the float staging buffer
            if ib is None:
                if pn is not None:
                    self._panorama = self._pan_result(h.pan(arr[0], kind, pn[0], pn[1]), kind, int(sample_rate), pn)
                _wide_in.HANDLE_CALLS[mod][0](h, arr, kind, int(sample_rate), src, dials, d_f32)
            else:
                d_ptr, n, self._input_blanker_stats = h.blank_in(arr[0], kind, *ib)
                if pn is not None:                                 # what the front end sees: the blanked samples, on the device
                    self._panorama = self._pan_result(h.pan(None, kind, pn[0], pn[1], d_ptr=d_ptr, n=n), kind, int(sample_rate), pn)
                _wide_in.HANDLE_CALLS[mod][3](h, d_ptr, n, kind, int(sample_rate), src, dials, d_f32)
            return self._decode_frames_locked(None, n_out, bands=bands, f32=f32, **args)

    @staticmethod
    def _pan_result(res, kind, rate, pn):
        """the one-shot's (rows, stats) as the dict of wide_in.WideIn.panorama: every row of the call, in order"""
        return {"data": res[0], "stats": res[1], "r_next": len(res[0]), "f_hz": _pan.freqs(kind, rate, pn[0]), "row_seconds": pn[0] * pn[1] / float(rate),
                "n_fft": pn[0], "n_avg": pn[1]}

    def _decode_frames_locked(self, audio, B, cyclestart_strings, return_records, passes, subtract_min_snr, sub_pass_osd, research="full",
                              recall=None, bands=None, f32=False):
        """audio None: the B frames are in the handle's staging buffer already (decode_stream); bands: per frame, instead of self.band;
        f32: float frames (float32 host frames, or the float staging buffer)"""
        if research not in ("full", "local"):
            raise _lib.Ft8rxError('research must be "full" or "local"')
        use_recall = self.recall or recall is not None
        on = _optins.active(self.cfg, recall=use_recall)
        if use_recall:
            _optins.refuse(_optins.RECALL, on)
        if int(passes) > 1:
            _optins.refuse(_optins.PASSES, on)
        h = self._handle(B)
        entries = self._recall_entries(recall if recall is not None else [None] * B) if use_recall else None
        res, rres, rp = self._pass(h, B, audio, entries, f32=f32)
        msgs, mcnt = self._package(res, rres)
        cs = [cyclestart_strings[f] if cyclestart_strings is not None else "700101_000015" for f in range(B)]
        band = [self.band] * B if bands is None else list(bands)
        out = [_m.message_dicts(msgs[f], mcnt[f], cyclestart_string=cs[f], band=band[f], odd_even=0, on_message=self.on_message,
                                ap=self._ap_on(), recall=use_recall, reports=None if rp is None else rp[f]) for f in range(B)]
        seen = [{" ".join(d["msg_tuple"]) for d in out[f]} for f in range(B)]

        def merge(p, msgs, mcnt):
            """the dict flavour: new texts only, tagged "_SUB", delivered in emit order; their rows compacted to the front of msgs"""
            keep = np.zeros(mcnt.shape, np.int32)
            for f in range(B):
                for i, d in enumerate(_m.message_dicts(msgs[f], mcnt[f], cyclestart_string=cs[f], band=band[f], odd_even=0)):
                    t = " ".join(d["msg_tuple"])
                    if t not in seen[f] and (sub_pass_osd or "OSD" not in d["decode_notes"]):
                        seen[f].add(t)
                        d["decode_notes"] += "_SUB"
                        out[f].append(d)
                        msgs[f, keep[f]] = msgs[f, i]                # compact: only the new messages are subtracted next
                        keep[f] += 1
                        if self.on_message is not None:
                            self.on_message(d)
            return msgs, keep
        rec, cnt = self._later_passes(h, B, passes, msgs, mcnt, res, subtract_min_snr, research == "local", merge, f32=f32)[:2]
        return (out, rec, cnt) if return_records else out

    @staticmethod
    def _subtraction_list(msgs, mcnt, rec, min_snr):
        """(signals[B, max] of _lib.SUBSIG_DTYPE, counts[B]): every emitted message with snr > min_snr, in emit order, with the
        tones of its codeword and the decoder's origin (fHz, tsec as the message dict reports them).  Native (ft8rx_subtraction_list);
        _subtraction_list_py is its numpy twin."""
        return _lib.subtraction_list(msgs, mcnt, rec, min_snr)

    @staticmethod
    def _subtraction_list_py(msgs, mcnt, rec, min_snr):
        B = len(mcnt)
        col = np.arange(msgs.shape[1])[None, :]
        sel = (col < np.asarray(mcnt)[:, None]) & (msgs["snr"] > min_snr)
        cnt = sel.sum(axis=1).astype(np.int32)
        ms = max(1, int(cnt.max()) if B else 1)
        arr = np.zeros((B, ms), _lib.SUBSIG_DTYPE)
        fi, mi = np.nonzero(sel)                                   # row-major: emit order within each frame
        if len(fi) == 0:
            return arr, cnt
        m = msgs[fi, mi]
        r = rec[fi, m["cand"]]
        slot = np.concatenate([np.arange(c) for c in cnt])
        fine = m["fine"] != 0
        arr["tones"][fi, slot] = _lib.encode_tones(r["msg_lo"], r["msg_hi"])
        arr["fHz"][fi, slot] = 3.125 * m["f0_idx"] + np.where(fine, m["ftweak"] / 16.0, 0.0)
        arr["tsec"][fi, slot] = m["h0_idx"] / 25.0 + np.where(fine, m["ttweak"] / 200.0, 0.0)
        return arr, cnt

    def decode_frames_arrays(self, audio_i16, n_threads=None, passes=1, subtract_min_snr=-10, sub_pass_osd=True, research="full",
                             float_frames=None):
        """High-throughput variant of decode_frames: no Python dicts.  -> (messages[B, 128] of _lib.MESSAGE_DTYPE,
        counts[B], records[B, max_cands], record_counts[B]); rows are in the reference's emit order.  With passes > 1 (see
        decode_frames) the messages of the later passes are appended per frame and carry the pass index (1, 2, ...) in
        messages["pad"][:, :, 0]; the returned records are those of the first pass.  float_frames: as decode_frames."""
        f32 = self._float_frames(float_frames)
        audio = _as_frames_f32(audio_i16) if f32 else _as_frames(audio_i16)
        B = audio.shape[0]
        if B == 0:
            raise _lib.Ft8rxError("empty batch")
        if research not in ("full", "local"):
            raise _lib.Ft8rxError('research must be "full" or "local"')
        _optins.refuse(_optins.ARRAYS, _optins.active(self.cfg))
        with self._hlock:
            h = self._handle(B)
            res = self._pass(h, B, audio, None, f32=f32)[0]
            msgs, mcnt = _lib.package_batch(*res, n_threads=n_threads)
            if passes > 1:
                # the array flavour of the merge is native (appends in place, up to the width of `out`)
                out, ocnt = msgs.copy(), np.ascontiguousarray(mcnt, np.int32).copy()
                self._later_passes(h, B, passes, msgs, mcnt, res, subtract_min_snr, research == "local",
                                   lambda p, m2, c2: _lib.merge_messages(out, ocnt, m2, c2, p, drop_osd=not sub_pass_osd), f32=f32,
                                   n_threads=n_threads)
                msgs, mcnt = out, ocnt
            return msgs, mcnt, res[0], res[1]

    def decode_frame(self, audio_i16, cyclestart_string="700101_000015", float_frames=None):
        return self.decode_frames(np.asarray(audio_i16)[None], [cyclestart_string], float_frames=float_frames)[0]

    def decode_frames_ft4(self, audio_i16, cyclestart_strings=None, return_records=False, passes=1, float_frames=None):
        """FT4 (extension): audio_i16 [B, 90000] int16, 7.5-s frames at 12 kHz -> per frame the list of message
        dicts (the keys of decode_frames, "mode": "FT4"; ft4.message_dicts), and the records / counts if asked.  Honours max_cands,
        search_freq_range, search_time_range (absolute start seconds; FT4's default is -0.5 .. +2.0), msg_types, ft4_sync_min and
        ft4_osd_max_hd; a fresh call-hash table per frame (and per pass).  The receiver's ft4_passes = 2 or 3 (section 19.6): the decoded
        signals are subtracted on the device and the residual is decoded again; the later passes' messages follow pass 1's, "_SUB" in
        their decode_notes, and the records returned are the last pass's.  The receiver's ft4_coherent=True (section 19.8): what BP
        leaves undecoded is decoded again on LLRs over runs of two and four symbols, and every dict says "nsym": 1, 2 or 4.  The
        receiver's ft4_weak=True (section 19.10): the candidates come from the coherent search on the 2.6-Hz grid; the dicts are unchanged.  The
        receiver's ft4_coh_osd=True (section 19.11, with ft4_coherent): OSD also runs on the coherent rows, gated by a whole-message score;
        such a message's "nsym" says 2 or 4.  The
        receiver's ft4_reports=True (section 19.9): every dict carries "report": {"snr", "fHz", "tsec"} measured on the audio its pass
        decoded (None where it could not be measured).  Refused, by name: a-priori calls, recall, weak, reports,
        the packed output, the per-call passes > 1 and float frames."""
        if (self.float_frames if float_frames is None else bool(float_frames)):
            raise _lib.Ft8rxError("FT4 decoding (decode_frames_ft4) is not supported together with float_frames=True: FT4 frames are int16")
        if int(passes) > 1:
            raise _lib.Ft8rxError(f"FT4 decoding (decode_frames_ft4) is not supported together with {_optins.TABLE[_optins.PASSES][0]}")
        _optins.refuse(_optins.FT4, _optins.active(self.cfg, recall=self.recall))
        audio = np.ascontiguousarray(audio_i16, np.int16) if not isinstance(audio_i16, (list, tuple)) else np.stack([np.asarray(a, np.int16) for a in audio_i16])
        if audio.ndim == 1:
            audio = audio[None]
        if audio.ndim != 2 or audio.shape[1] != _lib.FT4_NSAMP or len(audio) < 1:
            raise _lib.Ft8rxError(f"decode_frames_ft4: audio must be int16 [n_frames, {_lib.FT4_NSAMP}] (7.5 s at 12 kHz); got shape {audio.shape}")
        B = len(audio)
        with self._hlock:
            h = self._handle(B)
            gate = self._ft4_set(h)
            res = h.ft4_decode(audio)
            msgs, mcnt = self._package(res)
            cs = [cyclestart_strings[f] if cyclestart_strings is not None else "700101_000000" for f in range(B)]
            rp = self._ft4_measure(h, B, res[0], msgs, mcnt)
            if self.ft4_passes > 1:                                  # the later passes need the handle: the dicts are made under its lock
                out = [_ft4.message_dicts(msgs[f], mcnt[f], cyclestart_string=cs[f], band=self.band, on_message=self.on_message,
                                          nsym=self._ft4_nsym(res[0], msgs, mcnt, f), **self._ft4_rp(rp, f)) for f in range(B)]
                res = self._later_passes_ft4(h, B, res, msgs, mcnt, out, cs, gate)
                return (out, res[0], res[1]) if return_records else out
        out = [_ft4.message_dicts(msgs[f], mcnt[f], cyclestart_string=cs[f], band=self.band, on_message=self.on_message,
                                  nsym=self._ft4_nsym(res[0], msgs, mcnt, f), **self._ft4_rp(rp, f)) for f in range(B)]
        return (out, res[0], res[1]) if return_records else out

    def _ft4_measure(self, h, B, rec, msgs, mcnt, n_have=_lib.FT4_NSAMP):
        """ft4_reports: the measured reports (Handle.ft4_report) of the packaged messages of a batch whose frames
        lie in the handle's FT4 buffer (the caller holds its lock), of which the first n_have samples exist: one signal per message,
        from the record its row names -> per frame the REPORT_DTYPE rows, message by message; None with the setting off: nothing is
        called"""
        if not self.ft4_reports:
            return None
        n = [min(int(mcnt[f]), len(msgs[f])) for f in range(B)]
        sigs = np.zeros((B, max(1, max(n))), _lib.FT4_SUBSIG_DTYPE)
        rows = [rec[f][msgs[f]["cand"][:n[f]]] for f in range(B)]
        tones = _lib.ft4_encode_tones(np.concatenate([r["msg_lo"] for r in rows]), np.concatenate([r["msg_hi"] for r in rows]))
        at = 0
        for f, r in enumerate(rows):
            sigs[f, :n[f]]["start"] = _ft4.HOP * r["h0_idx"].astype(np.int32) + _ft4.DT_STEP * r["ttweak"].astype(np.int32)
            sigs[f, :n[f]]["fq"] = 4 * r["f0_idx"].astype(np.int32) + r["ftweak"].astype(np.int32)
            sigs[f, :n[f]]["tones"] = tones[at:at + n[f]]
            at += n[f]
        if not at:
            return [np.zeros(0, _lib.REPORT_DTYPE) for _ in range(B)]
        out = h.ft4_report(h.ft4_staging_ptr(), (sigs, np.asarray(n, np.int32)), n_have=n_have)
        return [out[f, :n[f]] for f in range(B)]

    @staticmethod
    def _ft4_rp(rp, f):
        """message_dicts' reports= of frame f; no keyword at all with the setting off"""
        return {} if rp is None else {"reports": rp[f]}

    def _ft4_set(self, h):
        """The receiver's FT4 knobs and search range on handle h (the caller holds its lock) -> the OSD gate in force"""
        # the OSD gate: the one given, else the library's default -- with msg_types set, the lower gate of the same noise sweep
        gate = self.ft4_osd_max_hd if self.ft4_osd_max_hd is not None or not self.cfg.msg_types else _ft4.OSD_MAX_HD_MSG_TYPES
        h.ft4_set(self.ft4_sync_min, gate)
        if self.ft4_coherent:                                        # a receiver without it never calls the setter: the handle's default is off
            h.ft4_set_coherent(True)
        if self.ft4_weak:                                            # likewise: never called without the keyword
            h.ft4_set_weak(True, self.ft4_weak_min)
        if self.ft4_coh_osd:                                         # likewise
            # the score gate: the one given, else the library's default -- with msg_types set, the stricter one measured for them
            ms = self.ft4_coh_osd_min_score if self.ft4_coh_osd_min_score is not None or not self.cfg.msg_types else _ft4.COH_OSD_MIN_SCORE_MSG_TYPES
            h.ft4_set_coh_osd(True, ms)
        f0 = _ft4.freq_range_to_f0(self._ft4_freq_range) if self._ft4_freq_range is not None else (0, 0)
        h0 = _ft4.time_range_to_h0(self._ft4_time_range) if self._ft4_time_range is not None else (0, 0)
        if f0 == (0, 0) and h0 != (0, 0):
            f0 = _ft4.freq_range_to_f0()
        if h0 == (0, 0) and f0 != (0, 0):
            h0 = _ft4.time_range_to_h0()
        h.ft4_set_range(f0[0], f0[1], h0[0], h0[1])
        return gate

    def _ft4_nsym(self, rec, msgs, mcnt, f):
        """ft4_coherent: per packaged message of frame f the run length its decode used -- the nsync of the candidate the row names, 0
        (a single-symbol decode) read as 1; None with the setting off: the dicts gain nothing"""
        if not self.ft4_coherent:
            return None
        return [int(v) or 1 for v in rec[f][msgs[f]["cand"][:int(mcnt[f])]]["nsync"]]

    @staticmethod
    def _ft4_words(rec, msgs, mcnt, f):
        """the 77-bit words of frame f's packaged messages, row by row (the word of the candidate a row names)"""
        r = rec[f][msgs[f]["cand"][:int(mcnt[f])]]
        return [(int(hi) << 64) | int(lo) for lo, hi in zip(r["msg_lo"], r["msg_hi"])]

    def _later_passes_ft4(self, h, B, res, msgs, mcnt, out, cs, gate, bands=None, notify=True, **pkg_kw):
        """Passes 2 .. ft4_passes of a batch whose frames pass 1 left in the handle's FT4 buffer: subtract the
        words that are new since the pass before (each once, in emit order, the start refined), decode the rounded residual with the
        unchanged chain, append the messages whose word the frame does not have yet ("_SUB" in decode_notes); stops when a pass brought
        nothing to subtract in any frame.  out: the per-frame dict lists, appended in place -> the results of the last pass run.
        The live pass (section 19.7): bands = one per frame, notify = False (on_message is its duplicate filter's business), pkg_kw =
        the persistent call-hash table."""
        have = [set(self._ft4_words(res[0], msgs, mcnt, f)) for f in range(B)]         # the words the frame's messages carry
        gone = [set() for _ in range(B)]                                               # the words already subtracted
        staging = h.ft4_staging_ptr()
        if self.ft4_sub_osd_max_hd is not None:
            h.ft4_set(self.ft4_sync_min, self.ft4_sub_osd_max_hd)
        try:
            for _ in range(1, self.ft4_passes):
                rec, cnt = res[0], res[1]
                sigs = _lib.ft4_subtraction_list(rec, cnt, gone)
                if not sigs[1].any():
                    break
                for f in range(B):
                    r = rec[f][:int(cnt[f])]
                    r = r[r["status"] == _lib.ST_DECODED]
                    gone[f].update((int(hi) << 64) | int(lo) for lo, hi in zip(r["msg_lo"], r["msg_hi"]))
                h.ft4_subtract(staging, B, sigs, refine=1)
                h.ft4_enqueue(staging, B)
                res = h.fetch(B)
                msgs, mcnt = self._package(res, **pkg_kw)
                rp = self._ft4_measure(h, B, res[0], msgs, mcnt)                       # on the residual this pass decoded
                for f in range(B):
                    words = self._ft4_words(res[0], msgs, mcnt, f)
                    for d, w in zip(_ft4.message_dicts(msgs[f], mcnt[f], cyclestart_string=cs[f], band=self.band if bands is None else bands[f],
                                                       nsym=self._ft4_nsym(res[0], msgs, mcnt, f), **self._ft4_rp(rp, f)), words):
                        if w in have[f]:
                            continue
                        have[f].add(w)
                        d["decode_notes"] += "_SUB"
                        out[f].append(d)
                        if notify and self.on_message is not None:
                            self.on_message(d)
        finally:
            if self.ft4_sub_osd_max_hd is not None:
                h.ft4_set(self.ft4_sync_min, gate)
        return res

    def decode_frame_ft4(self, audio_i16, cyclestart_string="700101_000000"):
        return self.decode_frames_ft4(np.asarray(audio_i16)[None], [cyclestart_string])[0]

    # ---- streaming mode (stands in for the manage_cycle thread, receiver.py:372-412)
    def _deliver(self, row, dicts, t0, early, seen_by_cycle, hist_by_cycle, out):
        """The tail of a live pass, for the 12 kHz path and for each channel of the wide path alike: `dicts` are the messages of the
        pass (`row`: their MESSAGE_DTYPE rows) for the cycle that starts at t0; early = hops of the cycle received so far, 0 = the
        complete frame.  Keeps the recall history (hist_by_cycle) and the per-cycle duplicate filter (seen_by_cycle), applies the
        early-pass filter and hands what is left to `out` and on_message."""
        if self.recall and not early:
            hist_by_cycle[t0] = dicts
            for k in [k for k in hist_by_cycle if k < t0 - 2 * T_CYC]:
                del hist_by_cycle[k]
        seen = seen_by_cycle.setdefault(t0, set())
        for k in [k for k in seen_by_cycle if k < t0 - 4 * T_CYC]:
            del seen_by_cycle[k]
        for i, d in enumerate(dicts):
            # early pass: only candidates whose PAYLOAD symbols (7..71) lie inside the hops received so far -- the reference's own
            # criterion for starting on a candidate (its search_grid_bounds, receiver.py:355,389; the last Costas block only
            # counts towards the sync gate) -- and no OSD decodes: first-CRC-valid-wins on a frame whose tail is padding
            # produces false decodes that the complete frame does not; what OSD finds is delivered by the end-of-cycle pass
            if early and (int(row[i]["h0_idx"]) + 4 + 4 * 72 + 4 > early or
                          int(row[i]["method"]) in (_lib.M_OSD, _lib.M_LDPC_B_OSD)):
                continue
            text = " ".join(d["msg_tuple"])
            if text in seen:                                       # the reference's per-cycle duplicate filter (receiver.py:52-54)
                continue
            seen.add(text)
            d["early"] = bool(early)
            out.append(d)
            if self.on_message is not None:
                self.on_message(d)

    def _live_pass(self, t0, early, K, frames, gather, bands, channels, seen, hist, out, f32=False):
        """One live pass over the K frames of the cycle that starts at t0 -- the 12 kHz path: K = 1, a host frame; the wide path: one
        frame per channel, which gather(h) brings into the live handle's staging buffer: decode them as one batch on the live handle,
        package with the persistent call-hash table (the frames are replayed into it in ascending order, package_batch(table=)) and
        deliver per frame (_deliver) with its band bands[j], its duplicate filter seen[j], its recall history hist[j] and -- channels
        not None -- "channel": channels[j].  f32: gather brings float frames into the float staging buffer."""
        cs = _time.strftime("%y%m%d_%H%M%S", _time.gmtime(t0))
        # recall: only the complete-frame pass, per frame the complete-frame messages of the same channel 30 s earlier (same parity),
        # and only when at least one frame has such a history
        prev = [hist[j].get(t0 - 2 * T_CYC) for j in range(K)] if self.recall and not early else None
        if prev is not None and all(p is None for p in prev):
            prev = None
        with self._live_lock:
            res, rres, rp = self._pass(self._live_handle(K), K, frames, None if prev is None else self._recall_entries(prev), gather, f32=f32)
        # the host message layer runs outside _live_lock: an audio callback that waits for a hop spectrum is not held up by it
        msgs, mcnt = self._package(res, rres, n_threads=1, table=self.call_hashes)
        for j in range(K):
            dicts = _m.message_dicts(msgs[j], mcnt[j], cyclestart_string=cs, band=bands[j], odd_even=int((t0 % (2 * T_CYC)) / T_CYC),
                                     ap=self._ap_on(), recall=self.recall, reports=None if rp is None else rp[j])
            if channels is not None:
                for d in dicts:
                    d["channel"] = channels[j]
            self._deliver(msgs[j], dicts, t0, early, seen[j], hist[j], out)

    def _deliver_ft4(self, rows, dicts, c, n_have, j, seen_by_slot, out):
        """The tail of a live FT4 pass for channel j and slot c: rows = the messages' MESSAGE_DTYPE rows in an early pass (n_have <
        90000: only what ft4.early_ok admits is delivered), None in the complete one; the per-slot duplicate filter on the text, slots
        older than four slots pruned"""
        early = n_have < _lib.FT4_NSAMP
        seen = seen_by_slot.setdefault(c, set())
        for k in [k for k in seen_by_slot if k < c - 4]:
            del seen_by_slot[k]
        for i, d in enumerate(dicts):
            if early and not _ft4.early_ok(int(rows[i]["h0_idx"]), int(rows[i]["ttweak"]), n_have):
                continue
            text = " ".join(d["msg_tuple"])
            if text in seen:
                continue
            seen.add(text)
            d["channel"], d["early"], d["their_tx_cycle"] = j, early, c % 2
            out.append(d)
            if self.on_message is not None:
                self.on_message(d)

    def _live_pass_ft4(self, w, c, m_first, n_have, out):
        """One live pass over the FT4 channels of the wide input for slot c (t = 7.5 c), of which n_have outputs
        exist: gather their 7.5-s frames into the live handle's FT4 buffer, decode them as one batch, package with the persistent
        call-hash table (the one the FT8 channels use) and deliver per channel.  The complete slot (n_have = 90000) runs the
        receiver's ft4_passes; an early pass is always single, and delivers only signals that lie wholly inside n_have."""
        ch = w.channels[_wide_in.FT4]
        B, early = len(ch), n_have < _lib.FT4_NSAMP
        cs = [_time.strftime("%y%m%d_%H%M%S", _time.gmtime(int(np.floor(_wide_in.FT4_T_SLOT * c))))] * B
        bands = [w.bands[j] if w.bands is not None else self.band for j in ch]
        pkg = dict(n_threads=1, table=self.call_hashes)
        dicts = None
        with self._live_lock:
            h = self._live_handle(w.n_channels)
            gate = self._ft4_set(h)
            h.ddc_stream_frames(m_first, n_have, _lib.FT4_NSAMP, ch)
            h.ft4_enqueue(h.ft4_staging_ptr(), B)
            res = h.fetch(B)
            later = not early and self.ft4_passes > 1
            if later or self.ft4_reports:                            # the later passes and the reports need the handle: packaged under its lock
                msgs, mcnt = self._package(res, **pkg)
                rp = self._ft4_measure(h, B, res[0], msgs, mcnt, n_have=n_have)       # an early pass: on the samples received
                dicts = [_ft4.message_dicts(msgs[f], mcnt[f], cyclestart_string=cs[f], band=bands[f], nsym=self._ft4_nsym(res[0], msgs, mcnt, f),
                                            **self._ft4_rp(rp, f)) for f in range(B)]
            if later:
                self._later_passes_ft4(h, B, res, msgs, mcnt, dicts, cs, gate, bands=bands, notify=False, **pkg)
        if dicts is None:                                            # the host message layer runs outside _live_lock
            msgs, mcnt = self._package(res, **pkg)
            dicts = [_ft4.message_dicts(msgs[f], mcnt[f], cyclestart_string=cs[f], band=bands[f], nsym=self._ft4_nsym(res[0], msgs, mcnt, f))
                     for f in range(B)]
        for f, j in enumerate(ch):
            self._deliver_ft4(msgs[f] if early else None, dicts[f], c, n_have, j, w.seen[j], out)

    def poll(self):
        """Decode every cycle that audio_in._callback has completed since the last call, then the passes of the wide input that have
        fallen due (wide_in.PassScheduler); messages go to on_message on the caller's thread.  -> list of message dicts.
        Receiver.start() runs this on a daemon thread (the stand-in for manage_cycle); without it, call poll() from your own loop
        (e.g. every 0.1 s).  Wide input: every dict carries "channel": j; band = bands[j]; fHz stays the audio frequency inside the
        channel.

        Unlike batched decode_frames (independent frames, a fresh call-hash table per frame), the stream is ONE receiver: the
        frames share the persistent table self.call_hashes, as the reference's process-global databases.call_hashes does
        (databases.py:8), so a hashed / non-standard call heard in cycle N resolves `<...>` in cycle N+1."""
        self._raise_thread_error()                                     # an exception on the audio / daemon thread surfaces here
        out = []
        while True:
            with self.audio_in._lock:
                if not self.audio_in._ready:
                    break
                frame, t_now, early = self.audio_in._ready.pop(0)           # early: hops of the cycle received so far, 0 = the complete frame
            # start of the cycle the frame belongs to: a full frame is handed over at its end, an early one inside it
            t0 = T_CYC * int(t_now / T_CYC) if early else T_CYC * int((t_now - T_CYC / 2) / T_CYC)
            self._live_pass(t0, early, 1, frame[None], None, [self.band], None, [self._cycle_seen], [self._recall_hist], out)
        w = self.wide_in
        while w is not None:
            with w._lock:
                if not w._ready:
                    break
                c, hop, m_first, n_have, *mode = w._ready.pop(0)
            if mode:                                                 # per-channel modes: the pass of one mode's channels
                if mode[0] == _wide_in.FT4:
                    self._live_pass_ft4(w, c, m_first, n_have, out)
                    continue
                ch = w.channels[_wide_in.FT8]
                self._live_pass(T_CYC * c, hop, len(ch), None, lambda h: h.ddc_stream_frames(m_first, n_have, _lib.NSAMP, ch),
                                [w.bands[j] if w.bands is not None else self.band for j in ch], ch, [w.seen[j] for j in ch],
                                [w.recall_hist[j] for j in ch], out)
                continue
            K = w.n_channels
            gather = (lambda h: h.ddc_stream_frame_f32(m_first, n_have)) if w.float_frames else (lambda h: h.ddc_stream_frame(m_first, n_have))
            self._live_pass(T_CYC * c, hop, K, None, gather,
                            w.bands if w.bands is not None else [self.band] * K, range(K), w.seen, w.recall_hist, out, f32=w.float_frames)
        return out


def decode_frames(audio_i16, on_message=None, passes=1, research="full", recall=None, float_frames=False, **receiver_kwargs):
    """decode_frames(audio_i16[B,180000], **receiver_kwargs) -> list[list[message dict]]  (SURVEY.md 8b); passes > 1 adds the
    subtraction passes of Receiver.decode_frames; recall = per frame the message dicts decoded 30 s earlier (Receiver.decode_frames);
    noise_blanker= (None / True / a threshold k / a dict of threshold, guard, taper) goes to Receiver with the other keyword arguments:
    the frames are blanked on the GPU (ft8rx_blank_host) before the first pass.  float_frames=True: float32 / float64 frames at any level,
    decoded unrounded (Receiver.decode_frames)."""
    audio = _as_frames_f32(audio_i16) if float_frames else _as_frames(audio_i16)
    rx = Receiver("", on_message, max_frames=max(1, audio.shape[0]), recall=recall is not None, float_frames=bool(float_frames),
                  **receiver_kwargs)       # reports=True: "report" in every dict
    return rx.decode_frames(audio, passes=passes, research=research, recall=recall)


def decode_frames_ft4(audio_i16, on_message=None, **receiver_kwargs):
    """decode_frames_ft4(audio_i16[B, 90000], **receiver_kwargs) -> list[list[message dict]]: Receiver.decode_frames_ft4 on a receiver
    of its own (FT4); ft4_passes=, ft4_coherent=, ft4_weak=, ft4_coh_osd=, ft4_reports= and the other FT4 knobs go to Receiver with the keyword
    arguments."""
    audio = np.ascontiguousarray(audio_i16, np.int16)
    rx = Receiver("", on_message, max_frames=max(1, audio.shape[0] if audio.ndim == 2 else 1), **receiver_kwargs)
    try:
        return rx.decode_frames_ft4(audio)
    finally:
        rx.close()
