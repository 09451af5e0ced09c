"""ctypes binding of libft8rx.so (include/ft8rx.h).  There is NO CPU fallback: if the HIP library is
missing or no MI355X is visible, the product raises."""
import ctypes as C
import os
import subprocess
import weakref

import numpy as np

from . import _abi, optins

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FT8RX_LIB", os.path.join(HERE, "libft8rx.so"))   # FT8RX_LIB: A/B builds of the same ABI
# the same source with the wide layouts (-DFT8RX_WIDE, include/ft8rx.h): search_freq_range up to 5900 Hz (and up to 2048 candidates per
# frame, more than 1024 = every f0 bin of a range up to 3000 Hz); loaded only when a config asks for it
LIB_PATH_WIDE = os.environ.get("FT8RX_LIB_WIDE", os.path.join(HERE, "libft8rx_wide.so"))
SRC = os.path.join(HERE, "csrc", "ft8rx.hip")
# second translation unit: the FFT kernels (k_fine, k_spectrogram), compiled with the ILP scheduling strategy -- 3.9 % / 3 % faster for
# them, 56 % slower for k_bp, and the strategy is a per-translation-unit choice (csrc/ft8rx_ilp.hip, profiles/archive/r03_notes.md)
SRC_ILP = os.path.join(HERE, "csrc", "ft8rx_ilp.hip")
ILP_FLAGS = ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"]
# -fno-slp-vectorize: on gfx950 a v_pk_add/mul_f32 issues at exactly the cost of the two scalar ops it replaces (tools/ubench/valu_rate.hip,
# profiles/archive/r02_valu_rate.txt) while the packing costs ~1000 extra v_mov in k_fine: scalar code is 7 % faster there, bit-identical.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-Wno-unused-result",
               "-Wno-unused-value", "-fPIC", "-shared"]

NSAMP, GRID_ROWS, GRID_COLS, SPEC_BINS, MAX_CANDS, EVENT_CAP = 180000, 376, 976, 49152, 1024, 512
MIN_H0, MAX_H0 = -898, 578                          # FT8RX_MIN_H0 / FT8RX_MAX_H0: bounds of config.h0_lo / h0_hi = where the reference's own search stops
                                                    # indexing its 750-row grid (search_time_range -36.4 .. +22.6 s, receiver.py:346-347)
MIN_H0_FD, MAX_H0_FD = -140, 220                    # FT8RX_MIN_H0_FD / _MAX_H0_FD: candidates inside take the frequency-domain fine sync
MAX_F0, GRID_COLS_WIDE, SPEC_BINS_WIDE, MAX_F0_WIDE = 960, 1920, 96000, 1888      # Handle.grid_cols / .spec_bins hold the loaded variant's
LADDER_GRID_CAP = 4 * 256 * 32                      # csrc/ft8rx.hip: the compiled grid cap of the ladder kernels (Handle.set_ladder_grid)
MAX_CANDS_WIDE = 2048                               # FT8RX_MAX_CANDS of the wide build: more than any search range has f0 bins
FT4_NSAMP, FT4_ROWS, FT4_COLS = 90000, 618, 577     # FT8RX_FT4_*: 7.5-s frames and their dB grid, the same in both builds


class Config(C.Structure):
    _fields_ = [("sync_score_min", C.c_float), ("max_cands", C.c_int32),
                ("f0_lo", C.c_int32), ("f0_hi", C.c_int32), ("h0_lo", C.c_int32), ("h0_hi", C.c_int32),
                ("bp_nc0_a", C.c_int32), ("bp_iters_a", C.c_int32), ("bp_nc0_b", C.c_int32), ("bp_iters_b", C.c_int32),
                ("osd_single", C.c_int32), ("osd_double", C.c_int32), ("llr_sd_min", C.c_float),
                ("osd_triple", C.c_int32), ("osd_max_hd", C.c_int32)]
    # opt-in message types (FT8RX_MT_* bits): not a field of ft8rx_config but a handle setting (ft8rx_set_msg_types) that Handle applies
    # at create time; kept here so that a config carries every knob of a receiver.  0 = the reference's rule.
    msg_types = 0
    # opt-in a-priori calls (ft8rx_set_ap_calls / ft8rx_set_ap_max_hd): handle settings too, applied by Handle at create time.
    # None = unset; both unset = the reference's ladder.
    ap_my_call = None
    ap_dx_call = None
    ap_max_hd = None                 # None = the library's default (FT8RX_AP_MAX_HD_DEFAULT)
    # recall (ft8rx_set_recall, ipass 8): entries are set per batch; this flag only marks a receiver that uses them (refusals)
    recall = False
    # opt-in weak-signal sync (ft8rx_set_weak): a handle setting too, applied by Handle at create time.
    # None = the library's defaults (FT8RX_WEAK_SYNC_MIN_DEFAULT / FT8RX_WEAK_OSD_MAX_HD_DEFAULT)
    weak = False
    weak_sync_min = None
    weak_osd_max_hd = None
    # opt-in measured reports (ft8rx_set_reports): a handle setting too, applied by Handle at create time
    reports = False


RECORD_DTYPE = np.dtype([("msg_lo", "<u8"), ("msg_hi", "<u8"), ("score", "<f4"), ("grid_sd", "<f4"), ("fine_sd", "<f4"),
                         ("f0_idx", "<i2"), ("h0_idx", "<i2"), ("ttweak", "i1"), ("ftweak", "i1"), ("snr_grid", "i1"),
                         ("snr_fine", "i1"), ("status", "u1"), ("ipass", "u1"), ("ap", "u1"), ("method", "u1"),
                         ("n_its", "<i2"), ("nsync", "u1"), ("osd_hd", "u1"), ("pad2", "<u4")])
EVENT_DTYPE = np.dtype([("msg_lo", "<u8"), ("msg_hi", "<u8"), ("cand", "<u2"), ("ipass", "u1"), ("slot", "u1"),
                        ("seq", "<u2"), ("valid", "<u2")])
MESSAGE_DTYPE = np.dtype([("f", "S16", (3,)), ("cand", "<i2"), ("f0_idx", "<i2"), ("h0_idx", "<i2"), ("snr", "i1"), ("ttweak", "i1"),
                          ("ftweak", "i1"), ("ipass", "u1"), ("ap", "u1"), ("method", "u1"), ("fine", "u1"), ("pad", "u1", (3,))])
# ft8rx_message_ext (ft8rx_package_batch_ext): wider text fields and the message type (i3, n3)
MESSAGE_EXT_DTYPE = np.dtype([("f", "S32", (3,)), ("cand", "<i2"), ("f0_idx", "<i2"), ("h0_idx", "<i2"), ("snr", "i1"), ("ttweak", "i1"),
                              ("ftweak", "i1"), ("ipass", "u1"), ("ap", "u1"), ("method", "u1"), ("fine", "u1"), ("i3", "u1"), ("n3", "u1"),
                              ("pad", "u1", (1,))])
assert MESSAGE_EXT_DTYPE.itemsize == 112
# Config.msg_types bits (include/ft8rx.h FT8RX_MT_*, ft8rx_set_msg_types)
MSG_TYPE_BITS = {"free_text": 1, "dxpedition": 2, "field_day": 4, "telemetry": 8, "rtty_ru": 16, "eu_vhf": 32}
MT_ALL = 63
SUBSIG_DTYPE = np.dtype([("fHz", "<f8"), ("tsec", "<f8"), ("tones", "u1", (79,)), ("pad", "u1")])
assert SUBSIG_DTYPE.itemsize == 96
FT4_SUBSIG_DTYPE = np.dtype([("start", "<i4"), ("fq", "<i4"), ("tones", "u1", (105,)), ("pad", "u1", (7,))])     # ft8rx_ft4_subsig
assert FT4_SUBSIG_DTYPE.itemsize == 120
# packed results (include/ft8rx.h: ft8rx_packed_header / ft8rx_packed_frame): header | frame table | kept records | used events
PACKED_MAGIC = 0x50385446
PACKED_HEADER_DTYPE = np.dtype([("magic", "<u4"), ("n_frames", "<i4"), ("n_records", "<i4"), ("n_events", "<i4"), ("bytes", "<u8"),
                                ("max_cands", "<i4"), ("overflow", "<i4")])
PACKED_FRAME_DTYPE = np.dtype([("rec_off", "<i4"), ("ev_off", "<i4"), ("n_cand", "<u2"), ("n_rec", "<u2"), ("n_ev", "<i4")])
assert PACKED_HEADER_DTYPE.itemsize == 32 and PACKED_FRAME_DTYPE.itemsize == 16
assert RECORD_DTYPE.itemsize == 48 and EVENT_DTYPE.itemsize == 24 and MESSAGE_DTYPE.itemsize == 64

ST_ACTIVE, ST_DECODED, ST_STOP_GRID_SD, ST_STOP_COSTAS, ST_STOP_FINE_SD, ST_EXHAUSTED = range(6)
M_AP_CODEWORD = 5                    # ipass 7, full pattern (include/ft8rx.h FT8RX_M_AP_CODEWORD)
AP_MAX_HD_DEFAULT = 36               # FT8RX_AP_MAX_HD_DEFAULT
WEAK_SYNC_MIN_DEFAULT = 148.5        # FT8RX_WEAK_SYNC_MIN_DEFAULT
WEAK_OSD_MAX_HD_DEFAULT = 30         # FT8RX_WEAK_OSD_MAX_HD_DEFAULT
# ipass-7 patterns (record field ap = 5 .. 10, ft8rx_set_ap_calls): name, calls it needs
AP_CALL_PATTERNS = {5: ("MY ???", "my"), 6: ("MY DX ???", "both"), 7: ("CQ DX ???", "dx"),
                    8: ("MY DX RRR", "both"), 9: ("MY DX 73", "both"), 10: ("MY DX RR73", "both")}
M_GOOD91, M_LDPC_A, M_LDPC_B, M_OSD, M_LDPC_B_OSD = range(5)
# recall of stations heard 30 s earlier (ft8rx_set_recall, ipass 8; include/ft8rx.h)
M_RECALL = 6                         # FT8RX_M_RECALL
RECALL_MAX = 64                      # FT8RX_RECALL_MAX: entries per frame
RECALL_MAX_HD_DEFAULT, RECALL_MIN_GAP_DEFAULT = 46, 12      # FT8RX_RECALL_MAX_HD_DEFAULT / _MIN_GAP_DEFAULT
RECALL_CLASSES = ("repeat", "RRR", "RR73", "73", "report", "R-report")      # the record's ap field on ipass 8
RECALL_ENTRY_DTYPE = np.dtype([("msg_lo", "<u8"), ("msg_hi", "<u8"), ("f0_idx", "<i2"), ("h0_idx", "<i2"), ("ttweak", "i1"),
                               ("ftweak", "i1"), ("pad", "<u2")])
assert RECALL_ENTRY_DTYPE.itemsize == 24
# measured reports (ft8rx_set_reports; include/ft8rx.h ft8rx_report, FT8RX_RP_*)
REPORT_DTYPE = np.dtype([("snr_db", "<f4"), ("f_hz", "<f4"), ("t_sec", "<f4"), ("score", "<f4"), ("flags", "<u4"), ("pad", "<u4")])
assert REPORT_DTYPE.itemsize == 24
RP_MEASURED, RP_INVALID, RP_EDGE_T, RP_EDGE_F = 1, 2, 4, 8

_libs = {}
_reject_log = [None]                  # set_reject_log's current path: applied to builds loaded later as well


class Ft8rxError(RuntimeError):
    pass


def _build_one(path, extra=(), ilp_flags=None, verbose=False):
    """Two objects (different scheduling strategies), one shared library at `path`.  If the ILP unit does not compile WITH its
    scheduling flag -- a hidden LLVM option a ROCm update may rename -- it is retried without (results are bit-identical either way,
    the flag is worth ~3 % on two kernels); objects and stray compiler processes are cleaned up whatever happens."""
    flags = [f for f in HIPCC_FLAGS if f != "-shared"]
    ilp = list(ILP_FLAGS if ilp_flags is None else ilp_flags)
    objs = [path[:-3] + ".main.o", path[:-3] + ".ilp.o"]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    cmds = [["hipcc"] + flags + list(extra) + ["-c", "-o", objs[0], SRC],
            ["hipcc"] + flags + ilp + list(extra) + ["-c", "-o", objs[1], SRC_ILP]]
    link = ["hipcc", "--offload-arch=gfx950", "-fPIC", "-shared", "-o", path] + objs
    procs = []
    try:
        if verbose:
            for c in cmds + [link]:
                print(" ".join(c))
        procs = [subprocess.Popen(c) for c in cmds]
        rcs = [p.wait() for p in procs]
        if rcs[1] != 0 and ilp:
            import warnings
            warnings.warn(f"hipcc rejected the ILP unit with {' '.join(ilp)}; building it with the default scheduler", RuntimeWarning)
            cmds[1] = [a for a in cmds[1] if a not in ilp]
            rcs[1] = subprocess.call(cmds[1])
        for c, rc in zip(cmds, rcs):
            if rc != 0:
                raise subprocess.CalledProcessError(rc, c)
        subprocess.check_call(link)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
        for o in objs:
            if os.path.exists(o):
                os.remove(o)
    return path


def build(force=False, verbose=False):
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU): libft8rx.so and libft8rx_wide.so."""
    deps = [os.path.join(os.path.dirname(HERE), "include", "ft8rx.h")]
    for d, _, files in os.walk(os.path.join(HERE, "csrc")):            # ft8rx.hip + ft8_dev.h, ft8_tables.h, kernels/*.hpp, host_messages.hpp
        deps += [os.path.join(d, f) for f in files if f.endswith((".hip", ".h", ".hpp"))]
    newest = max(os.path.getmtime(d) for d in deps)
    todo = [(path, extra) for path, extra in ((LIB_PATH, []), (LIB_PATH_WIDE, ["-DFT8RX_WIDE"]))
            if force or not os.path.exists(path) or os.path.getmtime(path) < newest]
    if len(todo) == 2:                                       # both variants side by side (four compiler processes)
        import threading
        errs = []

        def run(path, extra):
            try:
                _build_one(path, extra, verbose=verbose)
            except Exception as e:
                errs.append(e)
        ts = [threading.Thread(target=run, args=t) for t in todo]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if errs:
            raise errs[0]
    else:
        for path, extra in todo:
            _build_one(path, extra, verbose=verbose)
    return LIB_PATH


def build_variant(path, extra=(), ilp_flags=None):
    """An alternative build of the library (same two-unit recipe) at `path`, e.g. build_variant("build/ab/x.so", ["-DFINE_TIMING"]) for
    A/B timing through FT8RX_LIB (tools/ab_full.sh) -- never the product path."""
    try:
        return _build_one(path, extra, ilp_flags)
    except subprocess.CalledProcessError as e:
        raise Ft8rxError(f"build_variant({path}) failed: {e}")


def lib(wide=False):
    """The loaded library; wide=True -> the build with the wide layouts (Handle picks it when cfg.f0_hi > 960, or cfg.max_cands > 1024,
    which only a range beyond 3000 Hz has bins for).  The host-only entry points (message layer, tone encoder, hash tables, defaults)
    are the same code in both and are taken from the default one."""
    wide = bool(wide)
    if wide not in _libs:
        path = LIB_PATH_WIDE if wide else LIB_PATH
        if not os.path.exists(path):
            raise Ft8rxError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(pyft8_amd has no CPU fallback)")
        # PyTorch-ROCm wheels bundle their own libamdhip64.so.7; libft8rx.so links the system one (/opt/rocm, same soname).  The
        # copy loaded first serves both: this library runs on either, torch only on its own -- so if torch is already imported,
        # let it load and initialise its runtime before ours is pulled in.
        import sys
        if "torch" in sys.modules:
            try:
                sys.modules["torch"].cuda.is_available()
            except Exception:
                pass
        L = C.CDLL(path)
        missing = _abi.declare(L)                            # every prototype of include/ft8rx.h, once (pyft8_amd/_abi.py)
        if missing:
            raise Ft8rxError(f"{path} does not export {', '.join(missing)}: it was built from older source, build it again")
        gc, sb, mf = C.c_int32(), C.c_int32(), C.c_int32()
        L.ft8rx_build_info(C.byref(gc), C.byref(sb), C.byref(mf))
        want = (GRID_COLS_WIDE, SPEC_BINS_WIDE, MAX_F0_WIDE) if wide else (GRID_COLS, SPEC_BINS, MAX_F0)
        if (gc.value, sb.value, mf.value) != want:
            raise Ft8rxError(f"{path} was built with layouts {(gc.value, sb.value, mf.value)}, expected {want}")
        mc, ec = C.c_int32(), C.c_int32()
        L.ft8rx_build_limits(C.byref(mc), C.byref(ec))
        if (mc.value, ec.value) != ((MAX_CANDS_WIDE if wide else MAX_CANDS), EVENT_CAP):
            raise Ft8rxError(f"{path} was built with capacities {(mc.value, ec.value)} (FT8RX_MAX_CANDS, FT8RX_EVENT_CAP)")
        _libs[wide] = L
        if _reject_log[0]:                                   # a reject log set before this build was loaded applies to it too
            L.ft8rx_set_reject_log(_reject_log[0].encode())
    return _libs[wide]


def default_config(**kw):
    c = Config()
    lib().ft8rx_default_config(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def device_pci_bus_id(device):
    """PCI address ("0000:c1:00.0") of HIP device `device` (ft8rx_device_pci_bus_id), or None."""
    buf = C.create_string_buffer(64)
    return buf.value.decode() if lib().ft8rx_device_pci_bus_id(int(device), buf, 64) == 0 else None


def fft_plans():
    ps = [(C.c_int32 * 8)() for _ in range(4)]
    lib().ft8rx_get_fft_plans(*ps)
    names = ["plan1920", "plan3200", "plan300", "plan320"]
    return {n: [x for x in p if x] for n, p in zip(names, ps)}


def _audio(audio, refusal):
    """Host audio -> C-contiguous int16 [n_frames, 180000]; one frame may come as a vector.  refusal: the caller's wording
    ({shape} = what was given instead)."""
    audio = np.ascontiguousarray(audio, np.int16)
    if audio.ndim == 1:
        audio = audio[None]
    if audio.ndim != 2 or audio.shape[1] != NSAMP:
        raise Ft8rxError(refusal.format(shape=audio.shape))
    return audio


def _audio_f32(audio, refusal):
    """Host float frames -> C-contiguous float32 [n_frames, 180000]; float64 is rounded to float32 once, any
    other dtype is refused (integers are the int16 path's)."""
    audio = np.asarray(audio)
    if audio.dtype not in (np.float32, np.float64):
        raise Ft8rxError(refusal.format(shape=f"dtype {audio.dtype}"))
    audio = np.ascontiguousarray(audio, np.float32)
    if audio.ndim == 1:
        audio = audio[None]
    if audio.ndim != 2 or audio.shape[1] != NSAMP:
        raise Ft8rxError(refusal.format(shape=audio.shape))
    return audio


def _keep_f32(keep_f32):
    """keep_f32 of the stream opens: False / True, or 2 = the stream runs float frames (FT8RX_DDC_KEEP_F32_FRAMES)"""
    return 2 if keep_f32 is not True and keep_f32 == 2 else (1 if keep_f32 else 0)


def _words(bits):
    """77-bit words (Python ints) -> (msg_lo, msg_hi) uint64 arrays, as the records hold them."""
    return np.array([b & (2 ** 64 - 1) for b in bits], np.uint64), np.array([b >> 64 for b in bits], np.uint64)


_PRE_WORD = {"ddc_wide": "wide", "ddc_rat": "rational"}      # a pre-stage stream in messages, by the module of its stage
_PRE_FIELD = {"ddc_wide": "_wds", "ddc_rat": "_rts"}         # ... and the Handle field that describes it while it is open


def _pre_module(name):
    """pyft8_amd.ddc_wide or pyft8_amd.ddc_rat (they import this module, so they are imported on use)"""
    import importlib
    return importlib.import_module("." + name, __package__)


class Handle:
    """One HIP device + stream + preallocated workspaces for up to max_frames frames."""

    def __init__(self, cfg=None, device=0, max_frames=1):
        self.cfg = cfg or default_config()
        self.wide = self.cfg.f0_hi > MAX_F0 or self.cfg.max_cands > MAX_CANDS      # beyond 3000 Hz / 1024 candidates: the wide build (include/ft8rx.h)
        L = self._L = lib(self.wide)
        self.grid_cols, self.spec_bins = (GRID_COLS_WIDE, SPEC_BINS_WIDE) if self.wide else (GRID_COLS, SPEC_BINS)
        self.max_frames = int(max_frames)
        self.device = int(device)
        self._h = C.c_void_p()
        self.ap_calls = (None, None)
        self._ds = None                    # the open down-converter stream: (kind, n_streams, n_out)
        self._bis = None                   # the open input blanker stream: its kind
        self._wds = None                   # the open wide stream (ddc_wide_stream_open): (kind, n_out); _ds then describes the stage behind it
        self._rts = None                   # the open rational stream (ddc_rat_stream_open): (kind, n_out); likewise (_PRE_FIELD: at most one of the two)
        rc = L.ft8rx_create(C.byref(self.cfg), self.device, self.max_frames, C.byref(self._h))
        if rc != 0:
            raise Ft8rxError(f"ft8rx_create failed ({rc}): {L.ft8rx_last_error(None).decode()}")
        if self.cfg.msg_types:
            self.set_msg_types(self.cfg.msg_types)
        if self.cfg.ap_max_hd is not None:
            self.set_ap_max_hd(self.cfg.ap_max_hd)
        if self.cfg.ap_my_call or self.cfg.ap_dx_call:
            self.set_ap_calls(self.cfg.ap_my_call, self.cfg.ap_dx_call)
        if self.cfg.weak:
            self.set_weak(True, self.cfg.weak_sync_min, self.cfg.weak_osd_max_hd)
        if self.cfg.reports:
            self.set_reports(True)

    def set_msg_types(self, mask):
        """ft8rx_set_msg_types: the opt-in message types (MT_* bits; 0 = the reference's rule) of the batches enqueued afterwards."""
        self._chk(self._L.ft8rx_set_msg_types(self._h, int(mask)), "ft8rx_set_msg_types")
        self.cfg.msg_types = int(mask)

    def set_reports(self, on):
        """ft8rx_set_reports: measured SNR / frequency / start time of every DECODED record for the batches enqueued afterwards
        (DESIGN.md section 14); fetch_reports hands them out."""
        self._chk(self._L.ft8rx_set_reports(self._h, int(bool(on))), "ft8rx_set_reports")
        self.cfg.reports = bool(on)

    def fetch_reports(self, B):
        """ft8rx_fetch_reports: reports [B, max_cands] of REPORT_DTYPE of the batch the last fetch / decode_batch handed out, indexed
        like its records (flags 0 = no report: the slot did not decode, or the batch ran with the setting off)."""
        rp = np.zeros((int(B), self.cfg.max_cands), REPORT_DTYPE)
        self._chk(self._L.ft8rx_fetch_reports(self._h, int(B), rp.ctypes.data), "ft8rx_fetch_reports")
        return rp

    def report_probe(self, spec, frame, f0_idx, h0_idx, ttweak, ftweak, words):
        """ft8rx_report_probe: the measurement step alone on cycle spectra spec [B, spec_bins] complex64 for n candidates (frame,
        f0_idx, h0_idx, ttweak, ftweak, 77-bit word as a Python int) -> reports [n] (REPORT_DTYPE)."""
        spec = np.ascontiguousarray(spec, np.complex64)
        if spec.ndim == 1:
            spec = spec[None]
        if spec.ndim != 2 or spec.shape[1] != self.spec_bins:
            raise Ft8rxError(f"report_probe: spec must be complex64 [n_frames, {self.spec_bins}]")
        cols = [np.ascontiguousarray(x, np.int32).reshape(-1) for x in (frame, f0_idx, h0_idx, ttweak, ftweak)]
        n = len(cols[0])
        words = [int(w) for w in words]
        if n < 1 or any(len(c) != n for c in cols) or len(words) != n:
            raise Ft8rxError("report_probe: one frame, f0_idx, h0_idx, ttweak, ftweak and word per candidate")
        lo, hi = _words(words)
        rp = np.zeros(n, REPORT_DTYPE)
        self._chk(self._L.ft8rx_report_probe(self._h, spec.ctypes.data, int(spec.shape[0]), n, *[c.ctypes.data for c in cols], lo.ctypes.data,
                                             hi.ctypes.data, rp.ctypes.data), "ft8rx_report_probe")
        return rp

    def set_weak(self, on, sync_min=None, osd_max_hd=None):
        """ft8rx_set_weak: weak-signal sync for the batches enqueued afterwards (None = the library's defaults)."""
        sm = WEAK_SYNC_MIN_DEFAULT if sync_min is None else float(sync_min)
        hd = WEAK_OSD_MAX_HD_DEFAULT if osd_max_hd is None else int(osd_max_hd)
        self._chk(self._L.ft8rx_set_weak(self._h, int(bool(on)), sm, hd), "ft8rx_set_weak")
        self.cfg.weak = bool(on)
        if on:
            self.cfg.weak_sync_min, self.cfg.weak_osd_max_hd = sync_min, osd_max_hd

    def set_ap_calls(self, my_call=None, dx_call=None):
        """ft8rx_set_ap_calls: the operator's own call and the DX station's call as ipass-7 a-priori bits (None / "" = unset); applies
        to batches enqueued afterwards."""
        self._chk(self._L.ft8rx_set_ap_calls(self._h, (my_call or "").encode(), (dx_call or "").encode()), "ft8rx_set_ap_calls")
        self.ap_calls = (my_call or None, dx_call or None)

    def ap_calls_probe(self, llr):
        """ft8rx_ap_calls_probe: ipass 7 alone on fine-LLR vectors [n][174] (candidates 0 .. n - 1 of one frame) -> (records[n],
        events, event count)."""
        llr = np.ascontiguousarray(llr, np.float32).reshape(-1, 174)
        n = len(llr)
        rec = np.zeros(n, RECORD_DTYPE)
        ev = np.zeros(EVENT_CAP, EVENT_DTYPE)
        ne = C.c_int32(0)
        self._chk(self._L.ft8rx_ap_calls_probe(self._h, llr.ctypes.data, n, rec.ctypes.data, ev.ctypes.data, C.byref(ne)), "ft8rx_ap_calls_probe")
        return rec, ev, int(ne.value)

    def set_ap_max_hd(self, max_hd):
        self._chk(self._L.ft8rx_set_ap_max_hd(self._h, int(max_hd)), "ft8rx_set_ap_max_hd")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.ft8rx_destroy(self._h)
            self._h = C.c_void_p()
            self._packed_keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise Ft8rxError(f"{what} failed ({rc}): {self._L.ft8rx_last_error(self._h).decode()}")

    # ---- whole path
    def decode_batch(self, audio):
        audio = _audio(audio, f"audio must be int16 [n_frames, {NSAMP}] (15 s at 12 kHz); got shape {{shape}} -- see receiver.frames_from_ragged")
        if len(audio) < 1:
            raise Ft8rxError("empty batch")
        return self._run(audio, len(audio))

    def _alloc_out(self, B):
        # records / counts are written in full by the library; of the event rows only the used entries are (the rest must read as zero)
        mc = self.cfg.max_cands
        return (np.empty((B, mc), RECORD_DTYPE), np.empty(B, np.int32), np.zeros((B, EVENT_CAP), EVENT_DTYPE), np.empty(B, np.int32))

    def _run(self, audio, B):
        rec, cnt, ev, evc = self._alloc_out(B)
        self._chk(self._L.ft8rx_decode_batch(self._h, audio.ctypes.data, B, rec.ctypes.data, cnt.ctypes.data, ev.ctypes.data, evc.ctypes.data),
                  "ft8rx_decode_batch")
        return rec, cnt, ev, evc

    def decode_messages(self, audio, max_msgs=None, n_threads=None, table=None, return_flags=False):
        """ft8rx_decode_messages: host audio -> (messages[B, max_msgs] of MESSAGE_DTYPE, counts[B]) in one native call.  An
        overflowed event log or message list is warned about (Ft8rxTruncationWarning) and reported per frame with return_flags."""
        refusal = f"audio must be [n<={self.max_frames}, {NSAMP}] int16, got {{shape}}"
        audio = _audio(audio, refusal)
        if len(audio) > self.max_frames:
            raise Ft8rxError(refusal.format(shape=audio.shape))
        max_msgs = int(max_msgs or max(1, self.cfg.max_cands))
        res = _package("decode_messages", self._L.ft8rx_decode_messages, [self._h, audio.ctypes.data, len(audio)], len(audio), max_msgs,
                       n_threads or None, table, chk=self._chk)
        return res if return_flags else res[:2]

    # ---- float32 frames: the twins of the int16 entries around them
    def decode_batch_f32(self, audio):
        audio = _audio_f32(audio, f"audio must be float32 [n_frames, {NSAMP}] (15 s at 12 kHz); got {{shape}} -- see receiver.frames_from_ragged_f32")
        if len(audio) < 1:
            raise Ft8rxError("empty batch")
        B = len(audio)
        rec, cnt, ev, evc = self._alloc_out(B)
        self._chk(self._L.ft8rx_decode_batch_f32(self._h, audio.ctypes.data, B, rec.ctypes.data, cnt.ctypes.data, ev.ctypes.data, evc.ctypes.data),
                  "ft8rx_decode_batch_f32")
        return rec, cnt, ev, evc

    def decode_messages_f32(self, audio, max_msgs=None, n_threads=None, table=None, return_flags=False):
        """ft8rx_decode_messages_f32: decode_messages of float32 frames"""
        refusal = f"audio must be [n<={self.max_frames}, {NSAMP}] float32, got {{shape}}"
        audio = _audio_f32(audio, refusal)
        if len(audio) > self.max_frames:
            raise Ft8rxError(refusal.format(shape=audio.shape))
        max_msgs = int(max_msgs or max(1, self.cfg.max_cands))
        res = _package("decode_messages_f32", self._L.ft8rx_decode_messages_f32, [self._h, audio.ctypes.data, len(audio)], len(audio), max_msgs,
                       n_threads or None, table, chk=self._chk)
        return res if return_flags else res[:2]

    def enqueue_f32(self, d_audio_ptr, B):
        self._chk(self._L.ft8rx_enqueue_batch_f32(self._h, d_audio_ptr, int(B)), "ft8rx_enqueue_batch_f32")

    def enqueue_host_f32(self, audio):
        """enqueue_host of float32 frames (ft8rx_enqueue_batch_host_f32); the array stays alive and unchanged until the fetch"""
        if audio.dtype != np.float32 or audio.ndim != 2 or audio.shape[1] != NSAMP or not audio.flags["C_CONTIGUOUS"]:
            raise Ft8rxError(f"enqueue_host_f32: audio must be a C-contiguous float32 [n_frames, {NSAMP}] array")
        self._chk(self._L.ft8rx_enqueue_batch_host_f32(self._h, audio.ctypes.data, int(audio.shape[0])), "ft8rx_enqueue_batch_host_f32")

    def staging_ptr_f32(self):
        return int(self._L.ft8rx_staging_audio_f32(self._h) or 0)

    def download_audio_f32(self, d_ptr, n_frames):
        out = np.empty((n_frames, NSAMP), np.float32)
        self._chk(self._L.ft8rx_copy_to_host(self._h, out.ctypes.data, d_ptr, out.nbytes), "ft8rx_copy_to_host")
        return out

    def spectrogram_f32(self, audio):
        audio = _audio_f32(audio, f"spectrogram_f32: audio must be float32 [n_frames, {NSAMP}], got {{shape}}")
        g = np.empty((len(audio), GRID_ROWS, self.grid_cols), np.float32)
        self._chk(self._L.ft8rx_spectrogram_f32(self._h, audio.ctypes.data, len(audio), g.ctypes.data), "ft8rx_spectrogram_f32")
        return g

    def cycle_spectrum_f32(self, audio):
        audio = _audio_f32(audio, f"cycle_spectrum_f32: audio must be float32 [n_frames, {NSAMP}], got {{shape}}")
        s = np.empty((len(audio), self.spec_bins), np.complex64)
        self._chk(self._L.ft8rx_cycle_spectrum_f32(self._h, audio.ctypes.data, len(audio), s.ctypes.data), "ft8rx_cycle_spectrum_f32")
        return s

    def ddc_stream_frame_f32(self, m_first, n_have=NSAMP, d_audio_ptr=None):
        """Gather outputs [m_first, m_first + n_have) of every channel out of the float32 ring into the float staging audio (or d_audio_ptr)."""
        self._chk(self._L.ft8rx_ddc_stream_frame_f32(self._h, int(m_first) & 0xFFFFFFFFFFFFFFFF, int(n_have), d_audio_ptr), "ft8rx_ddc_stream_frame_f32")

    def enqueue(self, d_audio_ptr, B):
        self._chk(self._L.ft8rx_enqueue_batch(self._h, d_audio_ptr, int(B)), "ft8rx_enqueue_batch")

    def enqueue_host(self, audio):
        """Asynchronous decode of host audio (int16 [B, 180000], ideally from pinned_audio()): ft8rx_enqueue_batch_host.  The array
        must stay alive and unchanged until the batch has been fetched."""
        if audio.dtype != np.int16 or audio.ndim != 2 or audio.shape[1] != NSAMP or not audio.flags["C_CONTIGUOUS"]:
            raise Ft8rxError(f"enqueue_host: audio must be a C-contiguous int16 [n_frames, {NSAMP}] array")
        self._chk(self._L.ft8rx_enqueue_batch_host(self._h, audio.ctypes.data, int(audio.shape[0])), "ft8rx_enqueue_batch_host")

    def sync(self):
        self._chk(self._L.ft8rx_sync(self._h), "ft8rx_sync")

    def fetch(self, B, out=None):
        """ft8rx_fetch_results: the oldest unfetched batch's results, copied into fresh arrays -- or into `out` = a (rec, cnt, ev, evc)
        tuple an earlier call returned (a loop that fetches every few milliseconds then allocates nothing; event entries beyond
        the counts are stale in a reused set)."""
        rec, cnt, ev, evc = out if out is not None else self._alloc_out(B)
        if out is not None and (rec.shape != (B, self.cfg.max_cands) or ev.shape != (B, EVENT_CAP) or rec.dtype != RECORD_DTYPE or ev.dtype != EVENT_DTYPE
                                or cnt.shape != (B,) or evc.shape != (B,) or cnt.dtype != np.int32 or evc.dtype != np.int32
                                or not all(a.flags.c_contiguous and a.flags.writeable for a in (rec, cnt, ev, evc))):
            raise Ft8rxError("fetch: `out` is not a result set of this handle and batch size")
        self._chk(self._L.ft8rx_fetch_results(self._h, int(B), rec.ctypes.data, cnt.ctypes.data, ev.ctypes.data, evc.ctypes.data),
                  "ft8rx_fetch_results")
        return rec, cnt, ev, evc

    def fetch_view(self, B):
        """Like fetch, without the copy: numpy views of the handle's page-locked result buffers (ft8rx_fetch_results_view).
        Valid until two more batches have been enqueued."""
        B = int(B)
        p = [C.c_void_p() for _ in range(4)]
        self._chk(self._L.ft8rx_fetch_results_view(self._h, B, *[C.byref(x) for x in p]), "ft8rx_fetch_results_view")
        mc = self.cfg.max_cands

        def view(ptr, nbytes, dtype, shape):
            return np.frombuffer((C.c_char * nbytes).from_address(ptr.value), dtype=dtype).reshape(shape)
        return (view(p[0], B * mc * RECORD_DTYPE.itemsize, RECORD_DTYPE, (B, mc)), view(p[1], B * 4, np.int32, (B,)),
                view(p[2], B * EVENT_CAP * EVENT_DTYPE.itemsize, EVENT_DTYPE, (B, EVENT_CAP)), view(p[3], B * 4, np.int32, (B,)))

    def results_to_device(self, B, d_rec, d_cnt, d_ev, d_evc):
        """Latest batch's results -> caller-owned device buffers (raw device pointers; ft8rx_results_to_device)."""
        self._chk(self._L.ft8rx_results_to_device(self._h, int(B), d_rec, d_cnt, d_ev, d_evc), "ft8rx_results_to_device")

    def set_packed_output(self, buf0, buf1, cap_bytes, keep=None):
        """ft8rx_set_packed_output: raw pointers (device memory, or page-locked host memory from pinned_bytes()) of the two buffers the
        following batches write their packed results into (one per result slot); None, None turns it off.
        keep: the objects that own the two buffers (torch tensors, page-locked arrays).  The handle holds on to them -- and to the events
        given to packed_fence -- until the packed output is reset or the handle is closed, so the pack kernels can never write into
        memory whose Python owner has already been collected."""
        if buf0 is not None:          # (the library refuses the other settings itself; msg_types may be set in cfg alone)
            optins.refuse(optins.PACKED, optins.active(self.cfg) & {optins.MSG_TYPES})
        self._chk(self._L.ft8rx_set_packed_output(self._h, buf0 or None, buf1 or None, int(cap_bytes)), "ft8rx_set_packed_output")
        # (the call above has waited for every batch in flight: the previous owners may go now)
        self._packed_keep = {"buffers": keep, "fence": [None, None]} if (buf0 or buf1) else None

    def packed_fence(self, which, hip_event, keep=None):
        """ft8rx_packed_output_fence: the next batch that packs into buffer `which` waits (on the device) for this HIP event, e.g.
        torch.cuda.Event(...).cuda_event recorded behind an asynchronous send of the buffer.  keep: the object that owns the event."""
        self._chk(self._L.ft8rx_packed_output_fence(self._h, int(which), hip_event or None), "ft8rx_packed_output_fence")
        if getattr(self, "_packed_keep", None) is not None:
            self._packed_keep["fence"][int(which)] = keep

    def d2h_async(self, dst_ptr, src_ptr, nbytes):
        """ft8rx_d2h_async: device -> page-locked host copy on the handle's result-copy stream; -> ticket (d2h_done / d2h_event)."""
        t = C.c_int32()
        self._chk(self._L.ft8rx_d2h_async(self._h, dst_ptr, src_ptr, int(nbytes), C.byref(t)), "ft8rx_d2h_async")
        return int(t.value)

    def d2h_done(self, ticket):
        r = self._L.ft8rx_d2h_query(self._h, int(ticket))
        self._chk(min(r, 0), "ft8rx_d2h_query")
        return r == 1

    def d2h_event(self, ticket):
        return self._L.ft8rx_d2h_event(self._h, int(ticket))

    def packed_results(self):
        """ft8rx_packed_results: (which of the two packed buffers, its header as a dict) for the batch the last fetch returned."""
        which = C.c_int32()
        hdr = np.zeros(1, PACKED_HEADER_DTYPE)
        self._chk(self._L.ft8rx_packed_results(self._h, C.byref(which), hdr.ctypes.data), "ft8rx_packed_results")
        return int(which.value), {k: int(hdr[0][k]) for k in PACKED_HEADER_DTYPE.names}

    def pinned_bytes(self, nbytes):
        """uint8 array of page-locked host memory (ft8rx_alloc_host), released with the array."""
        L = self._L
        p = L.ft8rx_alloc_host(self._h, int(nbytes))
        if not p:
            raise Ft8rxError(f"ft8rx_alloc_host failed: {L.ft8rx_last_error(self._h).decode()}")
        buf = (C.c_uint8 * int(nbytes)).from_address(p)
        weakref.finalize(buf, L.ft8rx_free_host, None, p)
        return np.frombuffer(buf, dtype=np.uint8)

    def set_streams(self, n):
        self._chk(self._L.ft8rx_set_streams(self._h, int(n)), "ft8rx_set_streams")

    def set_subbatch(self, frames):
        """Frames per kernel chain inside a stream's share of a batch (ft8rx_set_subbatch; default 256, 0 = the whole share at once)."""
        self._chk(self._L.ft8rx_set_subbatch(self._h, int(frames)), "ft8rx_set_subbatch")

    def set_ladder_mode(self, mode):
        """0 (default) = fine-stage BP in ladder order, three launches (throughput); 1 = one launch for the five AP variants (latency)."""
        self._chk(self._L.ft8rx_set_ladder_mode(self._h, int(mode)), "ft8rx_set_ladder_mode")

    def set_ladder_grid(self, cap):
        """ft8rx_set_ladder_grid: the most blocks a ladder kernel is launched with (0 = the compiled default, LADDER_GRID_CAP; 1 ..
        LADDER_GRID_CAP is taken, anything else refused).  A test and tuning seam: results do not depend on it."""
        self._chk(self._L.ft8rx_set_ladder_grid(self._h, int(cap)), "ft8rx_set_ladder_grid")

    def set_search_mask(self, mask):
        """mask[n_frames, f0_hi - f0_lo] (non-zero = search this column, any score > 0) for the following batches, or None = the
        configured search again (ft8rx_set_search_mask: the subtraction experiment's local re-search)."""
        if mask is None:
            self._chk(self._L.ft8rx_set_search_mask(self._h, None, 0), "ft8rx_set_search_mask")
            return
        m = np.ascontiguousarray(mask, np.uint8)
        nf0 = self.cfg.f0_hi - self.cfg.f0_lo
        if m.ndim != 2 or m.shape[1] != nf0:
            raise Ft8rxError(f"set_search_mask: mask must be [n_frames, {nf0}]")
        self._chk(self._L.ft8rx_set_search_mask(self._h, m.ctypes.data, m.shape[0]), "ft8rx_set_search_mask")

    def set_recall(self, entries, counts=None):
        """ft8rx_set_recall: recall entries for the NEXT batch (ipass 8) -- entries [n_frames, RECALL_MAX] of
        RECALL_ENTRY_DTYPE with counts [n_frames], or a list (per frame) of RECALL_ENTRY_DTYPE arrays / lists of entries; None
        clears a pending setting.  The batch must have n_frames frames."""
        L = self._L
        if entries is None:
            self._chk(L.ft8rx_set_recall(self._h, None, None, 0), "ft8rx_set_recall")
            return
        if counts is None:
            rows = [np.asarray(e, RECALL_ENTRY_DTYPE).reshape(-1) for e in entries]
            if any(len(r) > RECALL_MAX for r in rows):
                raise Ft8rxError(f"set_recall: at most {RECALL_MAX} entries per frame")
            ent = np.zeros((len(rows), RECALL_MAX), RECALL_ENTRY_DTYPE)
            for f, r in enumerate(rows):
                ent[f, :len(r)] = r
            counts = [len(r) for r in rows]
        else:
            ent = np.ascontiguousarray(entries, RECALL_ENTRY_DTYPE)
        cnt = np.ascontiguousarray(counts, np.int32)
        if ent.ndim != 2 or ent.shape[1] != RECALL_MAX or cnt.shape != (ent.shape[0],):
            raise Ft8rxError(f"set_recall: entries must be [n_frames, {RECALL_MAX}] with counts [n_frames]")
        self._chk(L.ft8rx_set_recall(self._h, ent.ctypes.data, cnt.ctypes.data, int(ent.shape[0])), "ft8rx_set_recall")

    def fetch_recall(self, B):
        """ft8rx_fetch_recall: (records [B, RECALL_MAX] of RECORD_DTYPE, counts [B]) of the batch the last fetch / decode_batch handed
        out; record e belongs to entry e (zero where the entry was skipped)."""
        rec = np.zeros((int(B), RECALL_MAX), RECORD_DTYPE)
        cnt = np.zeros(int(B), np.int32)
        self._chk(self._L.ft8rx_fetch_recall(self._h, int(B), rec.ctypes.data, cnt.ctypes.data), "ft8rx_fetch_recall")
        return rec, cnt

    def set_recall_gates(self, max_hd=RECALL_MAX_HD_DEFAULT, min_gap=RECALL_MIN_GAP_DEFAULT):
        self._chk(self._L.ft8rx_set_recall_gates(self._h, int(max_hd), int(min_gap)), "ft8rx_set_recall_gates")

    def recall_probe(self, sgrid, entries):
        """ft8rx_recall_probe: k_recall_score alone on fine grids sgrid [n, 79, 8] for entries [n] -> records [n] (RECORD_DTYPE)."""
        sg = np.ascontiguousarray(sgrid, np.float32).reshape(-1, 632)
        ent = np.ascontiguousarray(entries, RECALL_ENTRY_DTYPE).reshape(-1)
        if len(ent) != len(sg):
            raise Ft8rxError("recall_probe: one grid per entry")
        rec = np.zeros(len(ent), RECORD_DTYPE)
        self._chk(self._L.ft8rx_recall_probe(self._h, sg.ctypes.data, ent.ctypes.data, len(ent), rec.ctypes.data), "ft8rx_recall_probe")
        return rec

    def set_profiling(self, on):
        self._L.ft8rx_set_profiling(self._h, int(bool(on)))

    def stage_times(self):
        n = C.c_int()
        names = (C.c_char_p * 24)()
        ms = (C.c_float * 24)()
        self._L.ft8rx_get_stage_times(self._h, C.byref(n), names, ms)
        return {names[i].decode(): ms[i] for i in range(n.value)}

    # ---- stage entry points
    def spectrogram(self, audio):
        audio = _audio(audio, f"spectrogram: audio must be int16 [n_frames, {NSAMP}], got shape {{shape}}")
        g = np.empty((len(audio), GRID_ROWS, self.grid_cols), np.float32)
        self._chk(self._L.ft8rx_spectrogram(self._h, audio.ctypes.data, len(audio), g.ctypes.data), "ft8rx_spectrogram")
        return g

    def hop_spectrum(self, window3840):
        w = np.ascontiguousarray(window3840, np.int16)
        if w.shape != (3840,):
            raise Ft8rxError(f"hop_spectrum needs the last 3840 samples, got shape {w.shape}")
        row = np.empty(self.grid_cols, np.float32)
        self._chk(self._L.ft8rx_hop_spectrum(self._h, w.ctypes.data, row.ctypes.data), "ft8rx_hop_spectrum")
        return row

    def _grid(self, grid):
        grid = np.ascontiguousarray(grid, np.float32)
        if grid.ndim == 2:
            grid = grid[None]
        if grid.shape[1:] != (GRID_ROWS, self.grid_cols):
            raise Ft8rxError(f"grid must be [n][{GRID_ROWS}][{self.grid_cols}] for this handle, got {grid.shape}")
        return grid

    def sync_search(self, grid):
        grid = self._grid(grid)
        B, mc = grid.shape[0], self.cfg.max_cands
        f0 = np.zeros((B, mc), np.int32); h0 = np.zeros((B, mc), np.int32); sc = np.zeros((B, mc), np.float32); cnt = np.zeros(B, np.int32)
        self._chk(self._L.ft8rx_sync_search(self._h, grid.ctypes.data, B, f0.ctypes.data, h0.ctypes.data, sc.ctypes.data, cnt.ctypes.data),
                  "ft8rx_sync_search")
        return f0, h0, sc, cnt

    def sync_scores(self, grid, f0_lo, f0_hi, weak=False):
        """ft8rx_sync_scores: per frame and f0 in [f0_lo, f0_hi) the best Costas score (first strict maximum over h0, from 0) and its h0.
        weak=True: ft8rx_sync_scores_weak, the score summed over all three Costas blocks (k_sync3)."""
        grid = self._grid(grid)
        B, n = grid.shape[0], int(f0_hi) - int(f0_lo)
        sc = np.zeros((B, max(n, 1)), np.float32); h0 = np.zeros((B, max(n, 1)), np.int32)
        name = "ft8rx_sync_scores_weak" if weak else "ft8rx_sync_scores"
        self._chk(getattr(self._L, name)(self._h, grid.ctypes.data, B, int(f0_lo), int(f0_hi), sc.ctypes.data, h0.ctypes.data), name)
        return sc, h0

    def llr_grid(self, grid, frame, f0, h0):
        grid = self._grid(grid)
        frame, f0, h0 = (np.ascontiguousarray(x, np.int32) for x in (frame, f0, h0))
        n = len(f0)
        llr = np.zeros((n, 174), np.float32); sd = np.zeros(n, np.float32); snr = np.zeros(n, np.int32)
        self._chk(self._L.ft8rx_llr_grid(self._h, grid.ctypes.data, grid.shape[0], n, frame.ctypes.data, f0.ctypes.data, h0.ctypes.data,
                                       llr.ctypes.data, sd.ctypes.data, snr.ctypes.data), "ft8rx_llr_grid")
        return llr, sd, snr

    def cycle_spectrum(self, audio):
        audio = _audio(audio, f"cycle_spectrum: audio must be int16 [n_frames, {NSAMP}], got shape {{shape}}")
        s = np.empty((len(audio), self.spec_bins), np.complex64)
        self._chk(self._L.ft8rx_cycle_spectrum(self._h, audio.ctypes.data, len(audio), s.ctypes.data), "ft8rx_cycle_spectrum")
        return s

    def fine(self, spec, frame, f0, h0, want_sgrid=False, weak=False):
        """ft8rx_fine (weak=True: ft8rx_fine_weak, the joint three-block scan of weak mode) for (frame, f0, h0) triples."""
        spec = np.ascontiguousarray(spec, np.complex64)
        if spec.ndim == 1:
            spec = spec[None]
        if spec.shape[1] != self.spec_bins:
            raise Ft8rxError(f"spectrum must be [n][{self.spec_bins}] for this handle, got {spec.shape}")
        frame, f0, h0 = (np.ascontiguousarray(x, np.int32) for x in (frame, f0, h0))
        n = len(f0)
        ret, tt, ft, ns, snr = (np.zeros(n, np.int32) for _ in range(5))
        llr = np.zeros((n, 174), np.float32); sd = np.zeros(n, np.float32)
        sg = np.zeros((n, 79, 8), np.float32) if want_sgrid else None
        name = "ft8rx_fine_weak" if weak else "ft8rx_fine"
        self._chk(getattr(self._L, name)(self._h, spec.ctypes.data, spec.shape[0], n, *[a.ctypes.data for a in (frame, f0, h0, ret, tt, ft, ns, llr, sd, snr)],
                                         sg.ctypes.data if want_sgrid else None), name)
        return dict(ret=ret, ttweak=tt, ftweak=ft, nsync=ns, llr=llr, sd=sd, snr=snr, sgrid=sg)

    def ldpc(self, llr, max_ncheck0, max_iters):
        llr = np.ascontiguousarray(llr, np.float32).reshape(-1, 174)
        n = len(llr)
        ok, nits, has = (np.zeros(n, np.int32) for _ in range(3))
        lo, hi = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        out = np.zeros((n, 174), np.float32)
        self._chk(self._L.ft8rx_ldpc(self._h, llr.ctypes.data, n, int(max_ncheck0), int(max_iters),
                                   *[a.ctypes.data for a in (ok, lo, hi, nits, has, out)]), "ft8rx_ldpc")
        return ok, lo, hi, nits, has, out

    def osd(self, llr, singleflips=30, doubleflips=2, tripleflips=0, max_hd=0, want_hd=False):
        llr = np.ascontiguousarray(llr, np.float32).reshape(-1, 174)
        n = len(llr)
        ok, trial, hd = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        lo, hi = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        self._chk(self._L.ft8rx_osd_ext(self._h, llr.ctypes.data, n, int(singleflips), int(doubleflips), int(tripleflips), int(max_hd),
                                      *[a.ctypes.data for a in (ok, lo, hi, trial, hd)]), "ft8rx_osd_ext")
        return (ok, lo, hi, trial, hd) if want_hd else (ok, lo, hi, trial)

    # ---- FT4 (7.5-s frames; DESIGN.md section 19, pyft8_amd/ft4.py)
    def _ft4_audio(self, audio, who):
        audio = np.ascontiguousarray(audio, np.int16)
        if audio.ndim == 1:
            audio = audio[None]
        if audio.ndim != 2 or audio.shape[1] != FT4_NSAMP or not 1 <= len(audio) <= self.max_frames:
            raise Ft8rxError(f"{who}: audio must be int16 [1 <= n <= {self.max_frames}, {FT4_NSAMP}] (7.5 s at 12 kHz); got shape {audio.shape}")
        return audio

    def ft4_set(self, sync_min=None, osd_max_hd=None):
        """ft8rx_ft4_set: the search threshold and OSD's distance gate of the FT4 batches enqueued afterwards (None = the default)."""
        self._chk(self._L.ft8rx_ft4_set(self._h, float(sync_min or 0.0), int(osd_max_hd or 0)), "ft8rx_ft4_set")

    def ft4_set_range(self, f0_lo=0, f0_hi=0, h0_lo=0, h0_hi=0):
        """ft8rx_ft4_set_range: bins [f0_lo, f0_hi) of 10.4167 Hz and rows [h0_lo, h0_hi) of 12 ms (ft4.freq_range_to_f0 /
        ft4.time_range_to_h0); all zero = the default, 12.5 .. 5900 Hz and -0.5 .. +2.0 s."""
        self._chk(self._L.ft8rx_ft4_set_range(self._h, int(f0_lo), int(f0_hi), int(h0_lo), int(h0_hi)), "ft8rx_ft4_set_range")

    def ft4_info(self):
        """ft8rx_ft4_info -> dict(workspace_bytes (0 until the handle's first FT4 call), sync_min, osd_max_hd, range)."""
        wb, sm, hd, rg = C.c_uint64(), C.c_float(), C.c_int32(), (C.c_int32 * 4)()
        self._chk(self._L.ft8rx_ft4_info(self._h, C.byref(wb), C.byref(sm), C.byref(hd), rg), "ft8rx_ft4_info")
        return dict(workspace_bytes=int(wb.value), sync_min=float(sm.value), osd_max_hd=int(hd.value), range=tuple(rg))

    def ft4_decode(self, audio):
        """ft8rx_ft4_decode_batch: host int16 [B, 90000] -> (records [B, max_cands], counts, events, event counts); FT4's record fields:
        include/ft8rx.h."""
        audio = self._ft4_audio(audio, "ft4_decode")
        B = len(audio)
        rec, cnt, ev, evc = self._alloc_out(B)
        self._chk(self._L.ft8rx_ft4_decode_batch(self._h, audio.ctypes.data, B, rec.ctypes.data, cnt.ctypes.data, ev.ctypes.data, evc.ctypes.data),
                  "ft8rx_ft4_decode_batch")
        return rec, cnt, ev, evc

    def ft4_enqueue(self, d_audio_ptr, B):
        self._chk(self._L.ft8rx_ft4_enqueue_batch(self._h, C.c_void_p(d_audio_ptr), int(B)), "ft8rx_ft4_enqueue_batch")

    def ft4_grid(self, audio, want_power=False):
        """ft8rx_ft4_grid -> dB [B, 618, 577] float32 (and the powers before the logarithm)."""
        audio = self._ft4_audio(audio, "ft4_grid")
        g = np.empty((len(audio), FT4_ROWS, FT4_COLS), np.float32)
        p = np.empty_like(g) if want_power else None
        self._chk(self._L.ft8rx_ft4_grid(self._h, audio.ctypes.data, len(audio), g.ctypes.data, p.ctypes.data if want_power else None), "ft8rx_ft4_grid")
        return (g, p) if want_power else g

    def ft4_sync(self, grid, want_best=False):
        """ft8rx_ft4_sync on dB grids [B, 618, 577] -> (f0, h0, score [B, max_cands], counts [B]) and, want_best, the per-bin maxima
        (best score, best h0) [B, f0_hi - f0_lo] before threshold and neighbour suppression."""
        grid = np.ascontiguousarray(grid, np.float32)
        if grid.ndim == 2:
            grid = grid[None]
        if grid.shape[1:] != (FT4_ROWS, FT4_COLS) or not 1 <= len(grid) <= self.max_frames:
            raise Ft8rxError(f"ft4_sync: grid must be [1 <= n <= {self.max_frames}][{FT4_ROWS}][{FT4_COLS}], got {grid.shape}")
        B, mc = len(grid), self.cfg.max_cands
        f0 = np.zeros((B, mc), np.int32); h0 = np.zeros((B, mc), np.int32); sc = np.zeros((B, mc), np.float32); cnt = np.zeros(B, np.int32)
        rg = self.ft4_info()["range"]
        bs = np.zeros((B, rg[1] - rg[0]), np.float32); bh = np.zeros((B, rg[1] - rg[0]), np.int32)
        self._chk(self._L.ft8rx_ft4_sync(self._h, grid.ctypes.data, B, f0.ctypes.data, h0.ctypes.data, sc.ctypes.data, cnt.ctypes.data,
                                         bs.ctypes.data if want_best else None, bh.ctypes.data if want_best else None), "ft8rx_ft4_sync")
        return (f0, h0, sc, cnt, bs, bh) if want_best else (f0, h0, sc, cnt)

    def ft4_demod(self, audio, frame, f0, h0):
        """ft8rx_ft4_demod: fine sync and demodulation of (frame, f0, h0) triples -> dict(ttweak, ftweak, metric, llr [n, 174], snr)."""
        audio = self._ft4_audio(audio, "ft4_demod")
        frame, f0, h0 = (np.ascontiguousarray(x, np.int32).reshape(-1) for x in (frame, f0, h0))
        n = len(f0)
        if n < 1 or len(frame) != n or len(h0) != n:
            raise Ft8rxError("ft4_demod: one frame, f0 and h0 per candidate")
        tw = np.zeros((n, 2), np.int32); met = np.zeros(n, np.float32); llr = np.zeros((n, 174), np.float32); snr = np.zeros(n, np.int32)
        self._chk(self._L.ft8rx_ft4_demod(self._h, audio.ctypes.data, len(audio), n, frame.ctypes.data, f0.ctypes.data, h0.ctypes.data,
                                          tw.ctypes.data, met.ctypes.data, llr.ctypes.data, snr.ctypes.data), "ft8rx_ft4_demod")
        return dict(ttweak=tw[:, 0].copy(), ftweak=tw[:, 1].copy(), metric=met, llr=llr, snr=snr)

    def ft4_set_coherent(self, on):
        """ft8rx_ft4_set_coherent: the coherent step (runs of two and four symbols) of the FT4 batches enqueued
        afterwards, on or off."""
        self._chk(self._L.ft8rx_ft4_set_coherent(self._h, 1 if on else 0), "ft8rx_ft4_set_coherent")

    def ft4_coh_info(self):
        """ft8rx_ft4_coh_info -> dict(workspace_bytes (0 until the first FT4 batch with the setting on), on)."""
        wb, on = C.c_uint64(), C.c_int32()
        self._chk(self._L.ft8rx_ft4_coh_info(self._h, C.byref(wb), C.byref(on)), "ft8rx_ft4_coh_info")
        return dict(workspace_bytes=int(wb.value), on=bool(on.value))

    def ft4_coherent(self, audio, frame, f0, h0, ttweak, ftweak):
        """ft8rx_ft4_coherent: k_ft4_coh on (frame, f0, h0) triples at the given fine-sync winners -> dict(q [n], metrics [n, 9],
        llr2, llr4 [n, 174])."""
        audio = self._ft4_audio(audio, "ft4_coherent")
        frame, f0, h0, tt, ft = (np.ascontiguousarray(x, np.int32).reshape(-1) for x in (frame, f0, h0, ttweak, ftweak))
        n = len(f0)
        if n < 1 or any(len(x) != n for x in (frame, h0, tt, ft)):
            raise Ft8rxError("ft4_coherent: one frame, f0, h0, ttweak and ftweak per candidate")
        q = np.zeros(n, np.int32); met = np.zeros((n, 9), np.float32); l2 = np.zeros((n, 174), np.float32); l4 = np.zeros((n, 174), np.float32)
        self._chk(self._L.ft8rx_ft4_coherent(self._h, audio.ctypes.data, len(audio), n, frame.ctypes.data, f0.ctypes.data, h0.ctypes.data,
                                             tt.ctypes.data, ft.ctypes.data, q.ctypes.data, met.ctypes.data, l2.ctypes.data, l4.ctypes.data),
                  "ft8rx_ft4_coherent")
        return dict(q=q, metrics=met, llr2=l2, llr4=l4)

    def ft4_set_weak(self, on, weak_min=None):
        """ft8rx_ft4_set_weak: the weak search (coherent Costas sync on the 2.6-Hz grid) of the FT4 batches
        enqueued afterwards, on or off, and its threshold (None = the default)."""
        self._chk(self._L.ft8rx_ft4_set_weak(self._h, 1 if on else 0, float(weak_min or 0.0)), "ft8rx_ft4_set_weak")

    def ft4_weak_info(self):
        """ft8rx_ft4_weak_info -> dict(workspace_bytes (0 until the first FT4 batch with the setting on), on, weak_min)."""
        wb, on, wm = C.c_uint64(), C.c_int32(), C.c_float()
        self._chk(self._L.ft8rx_ft4_weak_info(self._h, C.byref(wb), C.byref(on), C.byref(wm)), "ft8rx_ft4_weak_info")
        return dict(workspace_bytes=int(wb.value), on=bool(on.value), weak_min=float(wm.value))

    def ft4_sync_weak(self, audio, want_best=False):
        """ft8rx_ft4_sync_weak: the weak search's own launches on frames [B, 90000] -> (f0, h0, score [B, max_cands], counts [B]) and,
        want_best, the per-bin maxima (best score, best h0) [B, f0_hi - f0_lo] before threshold and neighbour suppression."""
        audio = self._ft4_audio(audio, "ft4_sync_weak")
        B, mc = len(audio), self.cfg.max_cands
        f0 = np.zeros((B, mc), np.int32); h0 = np.zeros((B, mc), np.int32); sc = np.zeros((B, mc), np.float32); cnt = np.zeros(B, np.int32)
        rg = self.ft4_info()["range"]
        bs = np.zeros((B, rg[1] - rg[0]), np.float32); bh = np.zeros((B, rg[1] - rg[0]), np.int32)
        self._chk(self._L.ft8rx_ft4_sync_weak(self._h, audio.ctypes.data, B, f0.ctypes.data, h0.ctypes.data, sc.ctypes.data, cnt.ctypes.data,
                                              bs.ctypes.data if want_best else None, bh.ctypes.data if want_best else None), "ft8rx_ft4_sync_weak")
        return (f0, h0, sc, cnt, bs, bh) if want_best else (f0, h0, sc, cnt)

    def ft4_set_coh_osd(self, on, min_score=None, max_hd=None):
        """ft8rx_ft4_set_coh_osd: OSD on the coherent rows behind the whole-message score of the FT4 batches
        enqueued afterwards that run the coherent step, on or off, and its two gates (None = the defaults)."""
        self._chk(self._L.ft8rx_ft4_set_coh_osd(self._h, 1 if on else 0, float(min_score or 0.0), int(max_hd or 0)), "ft8rx_ft4_set_coh_osd")

    def ft4_coh_osd_info(self):
        """ft8rx_ft4_coh_osd_info -> dict(workspace_bytes (0 until the first FT4 batch that runs the step), on, min_score, max_hd)."""
        wb, on, ms, hd = C.c_uint64(), C.c_int32(), C.c_float(), C.c_int32()
        self._chk(self._L.ft8rx_ft4_coh_osd_info(self._h, C.byref(wb), C.byref(on), C.byref(ms), C.byref(hd)), "ft8rx_ft4_coh_osd_info")
        return dict(workspace_bytes=int(wb.value), on=bool(on.value), min_score=float(ms.value), max_hd=int(hd.value))

    def ft4_verify(self, audio, frame, f0, h0, ttweak, ftweak, q, words, want_tones=False):
        """ft8rx_ft4_verify: k_ft4_verify on (frame, f0, h0) triples at the given fine-sync winners, residuals q and 77-bit words
        (Python ints) -> score [n] float32 (and, want_tones, the tones [n, 105] uint8 as the kernel encoded them)."""
        audio = self._ft4_audio(audio, "ft4_verify")
        frame, f0, h0, tt, ft, q = (np.ascontiguousarray(x, np.int32).reshape(-1) for x in (frame, f0, h0, ttweak, ftweak, q))
        n = len(f0)
        if n < 1 or any(len(x) != n for x in (frame, h0, tt, ft, q, words)):
            raise Ft8rxError("ft4_verify: one frame, f0, h0, ttweak, ftweak, q and word per candidate")
        lo = np.array([int(w) & (2 ** 64 - 1) for w in words], np.uint64)
        hi = np.array([int(w) >> 64 for w in words], np.uint64)
        sc = np.zeros(n, np.float32)
        tones = np.zeros((n, 105), np.uint8) if want_tones else None
        self._chk(self._L.ft8rx_ft4_verify(self._h, audio.ctypes.data, len(audio), n, frame.ctypes.data, f0.ctypes.data, h0.ctypes.data,
                                           tt.ctypes.data, ft.ctypes.data, q.ctypes.data, lo.ctypes.data, hi.ctypes.data, sc.ctypes.data,
                                           tones.ctypes.data if want_tones else None), "ft8rx_ft4_verify")
        return (sc, tones) if want_tones else sc

    def ft4_ldpc(self, llr, max_ncheck0, max_iters, mask=0):
        """ft8rx_ft4_ldpc: ldpc() on LLRs of FT4 codewords; the words come back descrambled."""
        llr = np.ascontiguousarray(llr, np.float32).reshape(-1, 174)
        n = len(llr)
        ok, nits, has = (np.zeros(n, np.int32) for _ in range(3))
        lo, hi = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        out = np.zeros((n, 174), np.float32)
        self._chk(self._L.ft8rx_ft4_ldpc(self._h, llr.ctypes.data, n, int(max_ncheck0), int(max_iters), int(mask),
                                         *[a.ctypes.data for a in (ok, lo, hi, nits, has, out)]), "ft8rx_ft4_ldpc")
        return ok, lo, hi, nits, has, out

    def ft4_osd(self, llr, singleflips=30, doubleflips=2, tripleflips=0, max_hd=0, mask=0):
        """ft8rx_ft4_osd: osd() on LLRs of FT4 codewords -> (ok, lo, hi, trial, hd); the words come back descrambled."""
        llr = np.ascontiguousarray(llr, np.float32).reshape(-1, 174)
        n = len(llr)
        ok, trial, hd = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        lo, hi = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        self._chk(self._L.ft8rx_ft4_osd(self._h, llr.ctypes.data, n, int(singleflips), int(doubleflips), int(tripleflips), int(max_hd), int(mask),
                                        *[a.ctypes.data for a in (ok, lo, hi, trial, hd)]), "ft8rx_ft4_osd")
        return ok, lo, hi, trial, hd

    def ft4_staging_ptr(self):
        """ft8rx_ft4_staging_audio: the device buffer where ft4_decode left the frames of its batch (0 before the first FT4 call)."""
        return int(self._L.ft8rx_ft4_staging_audio(self._h) or 0)

    def ft4_sub_info(self):
        """ft8rx_ft4_sub_info -> dict(workspace_bytes): 0 until the handle's first ft4_subtract / ft4_sub_probe."""
        wb = C.c_uint64()
        self._chk(self._L.ft8rx_ft4_sub_info(self._h, C.byref(wb)), "ft8rx_ft4_sub_info")
        return dict(workspace_bytes=int(wb.value))

    def ft4_subtract(self, d_audio_ptr, n_frames, signals, refine=1, return_float=False):
        """ft8rx_ft4_subtract on device-resident int16 frames [B, 90000], in place.  signals: (array [B, max_sigs] of FT4_SUBSIG_DTYPE,
        counts [B]), or per frame a list of (start, fq, tones105); subtracted in list order.  refine 1: the 13-trial start scan.
        -> (signals with the starts used, counts, the float32 residual before rounding or None)."""
        B = int(n_frames)
        if isinstance(signals, tuple):
            arr, cnt = signals
            arr = np.ascontiguousarray(arr, FT4_SUBSIG_DTYPE).copy()
            cnt = np.ascontiguousarray(cnt, np.int32)
        else:
            arr = np.zeros((B, max(1, max((len(s) for s in signals), default=1))), FT4_SUBSIG_DTYPE)
            cnt = np.zeros(B, np.int32)
            for f, lst in enumerate(signals):
                cnt[f] = len(lst)
                for i, (start, fq, tones) in enumerate(lst):
                    arr[f, i]["start"], arr[f, i]["fq"], arr[f, i]["tones"] = start, fq, np.asarray(tones, np.uint8)
        if arr.ndim != 2 or arr.shape[0] != B or len(cnt) != B:
            raise Ft8rxError(f"ft4_subtract: signals [n_frames = {B}][max_sigs] and one count per frame expected")
        out = np.empty((B, FT4_NSAMP), np.float32) if return_float else None
        self._chk(self._L.ft8rx_ft4_subtract(self._h, C.c_void_p(d_audio_ptr), B, arr.ctypes.data, cnt.ctypes.data, int(arr.shape[1]), int(refine),
                                             out.ctypes.data if return_float else None), "ft8rx_ft4_subtract")
        return arr, cnt, out

    def ft4_sub_probe(self, audio, frame, sigs, want_model=False):
        """ft8rx_ft4_sub_probe: signal i (FT4_SUBSIG_DTYPE) on frame frame[i] of the host frames -> dict(bins complex [n, 41] at the given
        start (index k + 20), energy [n, 13] of the refine trials, model complex64 [n, 60480] if asked)."""
        audio = self._ft4_audio(audio, "ft4_sub_probe")
        frame = np.ascontiguousarray(frame, np.int32).reshape(-1)
        sigs = np.ascontiguousarray(sigs, FT4_SUBSIG_DTYPE).reshape(-1)
        n = len(frame)
        if n < 1 or len(sigs) != n:
            raise Ft8rxError("ft4_sub_probe: one frame per signal")
        bins, en = np.zeros((n, 41), np.complex128), np.zeros((n, 13), np.float64)
        model = np.zeros((n, 60480), np.complex64) if want_model else None
        self._chk(self._L.ft8rx_ft4_sub_probe(self._h, audio.ctypes.data, len(audio), n, frame.ctypes.data, sigs.ctypes.data,
                                              model.ctypes.data if want_model else None, bins.ctypes.data, en.ctypes.data), "ft8rx_ft4_sub_probe")
        return dict(bins=bins, energy=en, model=model)

    def ft4_report_info(self):
        """ft8rx_ft4_report_info -> dict(workspace_bytes): 0 until the handle's first ft4_report."""
        wb = C.c_uint64()
        self._chk(self._L.ft8rx_ft4_report_info(self._h, C.byref(wb)), "ft8rx_ft4_report_info")
        return dict(workspace_bytes=int(wb.value))

    def ft4_report(self, audio, sigs, n_have=FT4_NSAMP, stages=False):
        """ft8rx_ft4_report: the measured reports (ft4.report is the twin) of decoded signals.  audio: a device
        pointer to int16 frames [B, 90000] (ft4_staging_ptr after an FT4 batch), or a host array, which is uploaded.  sigs: (array
        [B, max_sigs] of FT4_SUBSIG_DTYPE, counts [B]), or per frame a list of (start, fq, tones105).  Of each frame's samples only
        the first n_have exist.  -> REPORT_DTYPE [B, max_sigs] (all zero from a frame's count on); stages: (reports, scores
        [B, max_sigs, 13, 13], on_off [B, max_sigs, 2])."""
        if isinstance(sigs, tuple):
            arr, cnt = sigs
            arr = np.ascontiguousarray(arr, FT4_SUBSIG_DTYPE)
            cnt = np.ascontiguousarray(cnt, np.int32)
        else:
            arr = np.zeros((len(sigs), max(1, max((len(s) for s in sigs), default=1))), FT4_SUBSIG_DTYPE)
            cnt = np.zeros(len(sigs), np.int32)
            for f, lst in enumerate(sigs):
                cnt[f] = len(lst)
                for i, (start, fq, tones) in enumerate(lst):
                    arr[f, i]["start"], arr[f, i]["fq"], arr[f, i]["tones"] = start, fq, np.asarray(tones, np.uint8)
        if arr.ndim != 2 or len(cnt) != arr.shape[0]:
            raise Ft8rxError("ft4_report: signals [n_frames][max_sigs] and one count per frame expected")
        B, ms = arr.shape
        keep = None
        if isinstance(audio, (int, np.integer)):
            ptr = int(audio)
        else:
            host = self._ft4_audio(audio, "ft4_report")
            if len(host) != B:
                raise Ft8rxError(f"ft4_report: {len(host)} frames for {B} rows of signals")
            import torch
            keep = torch.from_numpy(host if host.flags.writeable else host.copy()).to(f"cuda:{self.device}")
            torch.cuda.synchronize(keep.device)
            ptr = keep.data_ptr()
        rep = np.zeros((B, ms), REPORT_DTYPE)
        sc = np.zeros((B, ms, 13, 13), np.float32) if stages else None
        oo = np.zeros((B, ms, 2), np.float32) if stages else None
        self._chk(self._L.ft8rx_ft4_report(self._h, C.c_void_p(ptr), int(B), arr.ctypes.data, cnt.ctypes.data, int(ms), int(n_have), rep.ctypes.data,
                                           sc.ctypes.data if stages else None, oo.ctypes.data if stages else None), "ft8rx_ft4_report")
        del keep
        return (rep, sc, oo) if stages else rep

    def download_audio_ft4(self, d_ptr, n_frames):
        out = np.empty((int(n_frames), FT4_NSAMP), np.int16)
        self._chk(self._L.ft8rx_copy_to_host(self._h, out.ctypes.data, C.c_void_p(d_ptr), out.nbytes), "ft8rx_copy_to_host")
        return out

    def crc_valid(self, cw91):
        cw91 = np.ascontiguousarray(cw91, np.float32).reshape(-1, 91)
        n = len(cw91)
        res = np.zeros(n, np.int32); lo, hi = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        self._chk(self._L.ft8rx_crc_valid(self._h, cw91.ctypes.data, n, res.ctypes.data, lo.ctypes.data, hi.ctypes.data), "ft8rx_crc_valid")
        return res, lo, hi

    def valid77(self, bits):
        lo, hi = _words(bits)
        out = np.zeros(len(lo), np.int32)
        self._chk(self._L.ft8rx_valid77(self._h, lo.ctypes.data, hi.ctypes.data, len(lo), out.ctypes.data), "ft8rx_valid77")
        return out

    def valid77_ext(self, bits, mask):
        """ft8rx_valid77_ext: the validity predicate with the opt-in message types `mask` (MSG_TYPE_BITS) on the GPU."""
        lo, hi = _words(bits)
        out = np.zeros(len(lo), np.int32)
        self._chk(self._L.ft8rx_valid77_ext(self._h, lo.ctypes.data, hi.ctypes.data, len(lo), int(mask), out.ctypes.data), "ft8rx_valid77_ext")
        return out

    def subtract(self, d_audio_ptr, n_frames, signals, return_float=False, refine=False, return_origins=False, float_frames=False):
        """Subtract decoded signals from device-resident int16 audio in place (ft8rx_subtract).
        signals: per frame a list of (tones79, fHz, tsec), subtracted in list order.  -> float32 residual if return_float.
        refine: 0 = as given (the reference's subtract_signal), 1 = re-estimate each origin first with full-rate scans, 2 = the same on
        a decimated baseband copy (fast; what Receiver's multi-pass decode uses).  float_frames: d_audio_ptr holds float32 frames, which
        are worked on and written back as they are (ft8rx_subtract_f32)."""
        B = int(n_frames)
        if isinstance(signals, tuple):          # (array [B, max_sigs] of SUBSIG_DTYPE, counts [B]) -- the fast path
            arr, cnt = signals
            arr = np.ascontiguousarray(arr, SUBSIG_DTYPE)
            cnt = np.ascontiguousarray(cnt, np.int32)
            ms = arr.shape[1]
        else:
            ms = max(1, max((len(s) for s in signals), default=1))
            arr = np.zeros((B, ms), SUBSIG_DTYPE)
            cnt = np.zeros(B, np.int32)
            for f, lst in enumerate(signals):
                cnt[f] = len(lst)
                for i, (tones, fHz, tsec) in enumerate(lst):
                    arr[f, i]["tones"] = np.asarray(tones, np.uint8)
                    arr[f, i]["fHz"], arr[f, i]["tsec"] = fHz, tsec
        out = np.empty((B, NSAMP), np.float32) if return_float else None
        entry = "ft8rx_subtract_f32" if float_frames else "ft8rx_subtract"
        self._chk(getattr(self._L, entry)(self._h, d_audio_ptr, B, arr.ctypes.data, cnt.ctypes.data, ms, int(refine),
                                          out.ctypes.data if return_float else None), entry)
        if return_origins:                 # (fHz, tsec) per signal after refinement
            return out, [[(float(arr[f, i]["fHz"]), float(arr[f, i]["tsec"])) for i in range(cnt[f])] for f in range(B)]
        return out

    def ddc(self, samples, kind, rate, src, f_dial_hz, gain=1.0, want_float=False, device=False, d_ptr=None, n=None, d_f32_ptr=None):
        """ft8rx_ddc_host / ft8rx_ddc: down-convert [n_streams][n] samples of `kind` (ddc.REAL_I16 .. ddc.IQ_F32;
        IQ as complex or (I, Q) pairs, ddc.pack) at `rate` Hz into len(src) frames in the staging buffer (staging_ptr, download_audio),
        output j = stream src[j] with the dial f_dial_hz[j] Hz from the stream's centre -> f_mixed_hz [n_out], the dials really mixed.
        want_float: -> (f_mixed_hz, y float32 [n_out, 180000]), the audio before rounding.  device / want_float: the samples go
        through a torch tensor and the device entry (ft8rx_ddc) instead of the library's own staging (ft8rx_ddc_host).  d_ptr, n: ONE
        stream of n samples that is on the device already (a raw address, what blank_in returns; `samples` is not looked at): the
        device entry on it, queued and not waited for.  d_f32_ptr: a device address [n_out][180000] float32 that receives the audio before
        rounding (float frames, DESIGN.md section 18: staging_ptr_f32()); the device entry, -> f_mixed_hz."""
        from . import ddc as _ddc
        if d_ptr is not None:
            src = np.ascontiguousarray(src, np.int32).reshape(-1)
            f = np.ascontiguousarray(f_dial_hz, np.float64).reshape(-1)
            if len(src) != len(f) or len(src) < 1:
                raise Ft8rxError(f"ddc: one src and one f_dial_hz per output, got {len(src)} and {len(f)}")
            fm = np.zeros(len(src), np.float64)
            self._chk(self._L.ft8rx_ddc(self._h, int(d_ptr), int(kind), int(rate), 1, int(n), int(n), len(src), src.ctypes.data, f.ctypes.data,
                                        float(gain), None, d_f32_ptr, fm.ctypes.data), "ft8rx_ddc")
            return fm
        a, n_streams, n = _ddc.pack(samples, kind)
        src = np.ascontiguousarray(src, np.int32).reshape(-1)
        f = np.ascontiguousarray(f_dial_hz, np.float64).reshape(-1)
        if len(src) != len(f) or len(src) < 1:
            raise Ft8rxError(f"ddc: one src and one f_dial_hz per output, got {len(src)} and {len(f)}")
        fm = np.zeros(len(src), np.float64)
        args = (int(kind), int(rate), n_streams, n, n, len(src), src.ctypes.data, f.ctypes.data, float(gain))
        if not (device or want_float or d_f32_ptr is not None):
            self._chk(self._L.ft8rx_ddc_host(self._h, a.ctypes.data, *args, fm.ctypes.data), "ft8rx_ddc_host")
            return fm
        import torch
        dev = torch.device("cuda", self.device)
        d_in = torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
        d_f32 = torch.empty((len(src), NSAMP), dtype=torch.float32, device=dev) if want_float else None
        torch.cuda.synchronize(dev)
        self._chk(self._L.ft8rx_ddc(self._h, d_in.data_ptr(), *args, None, d_f32.data_ptr() if want_float else d_f32_ptr, fm.ctypes.data), "ft8rx_ddc")
        self.sync()                                          # the tensors may go once the kernel has run
        return (fm, d_f32.cpu().numpy()) if want_float else fm

    # ---- streaming down-converter (ft8rx_ddc_stream_*): one stream set per handle, state on the device
    def ddc_stream_open(self, kind, rate, n_streams, src, f_dial_hz, gain=1.0, n_origin=0, keep_f32=False):
        """Open the stream: n_streams inputs of `kind` at `rate` Hz feed len(src) channels (channel j = stream src[j], dial
        f_dial_hz[j]); n_origin = absolute index of the first sample that will be pushed, a multiple of 1008 D.  -> f_mixed_hz."""
        src = np.ascontiguousarray(src, np.int32).reshape(-1)
        f = np.ascontiguousarray(f_dial_hz, np.float64).reshape(-1)
        if len(src) != len(f) or len(src) < 1:
            raise Ft8rxError(f"ddc_stream_open: one src and one f_dial_hz per channel, got {len(src)} and {len(f)}")
        fm = np.zeros(len(src), np.float64)
        self._chk(self._L.ft8rx_ddc_stream_open(self._h, int(kind), int(rate), int(n_streams), len(src), src.ctypes.data, f.ctypes.data,
                                                float(gain), int(n_origin), _keep_f32(keep_f32), fm.ctypes.data), "ft8rx_ddc_stream_open")
        self._ds = (int(kind), int(n_streams), len(src))
        return fm

    def ddc_stream_push(self, samples, d_ptr=None, n=None):
        """Push the next samples of every stream ([n_streams][n], forms of ddc.pack; 1 .. one second) -> absolute index one past the
        last output produced so far.  Asynchronous.  d_ptr, n: the n next samples of the ONE stream, on the device already."""
        from . import ddc as _ddc
        if self._ds is None:
            raise Ft8rxError("ddc_stream_push: no stream is open (ddc_stream_open)")
        if d_ptr is not None:
            if self._ds[1] != 1:
                raise Ft8rxError(f"ddc_stream_push: d_ptr carries one stream, the open stream has {self._ds[1]}")
            m = C.c_uint64()
            self._chk(self._L.ft8rx_ddc_stream_push(self._h, int(d_ptr), int(n), 1, C.byref(m)), "ft8rx_ddc_stream_push")
            return int(m.value)
        a, n_streams, n = _ddc.pack(samples, self._ds[0])
        if n_streams != self._ds[1]:
            raise Ft8rxError(f"ddc_stream_push: {n_streams} streams, the open stream has {self._ds[1]}")
        m = C.c_uint64()
        self._chk(self._L.ft8rx_ddc_stream_push(self._h, a.ctypes.data, n, 0, C.byref(m)), "ft8rx_ddc_stream_push")
        return int(m.value)

    def ddc_stream_frame(self, m_first, n_have=NSAMP, d_audio_ptr=None):
        """Gather outputs [m_first, m_first + n_have) of every channel into the frames of the staging buffer (or d_audio_ptr)."""
        self._chk(self._L.ft8rx_ddc_stream_frame(self._h, int(m_first) & 0xFFFFFFFFFFFFFFFF, int(n_have), d_audio_ptr), "ft8rx_ddc_stream_frame")

    def ddc_stream_frames(self, m_first, n_have, frame_len, channels=None, n_sel=None, d_audio_ptr=None):
        """ft8rx_ddc_stream_frames: outputs [m_first, m_first + n_have) of the channels `channels` (None = channels
        0 .. n_sel - 1, n_sel None = every channel of the stream) as frames of frame_len = NSAMP or FT4_NSAMP samples, into d_audio_ptr --
        None = the FT4 frame buffer (ft4_staging_ptr) for frame_len 90000, the staging buffer (staging_ptr) for 180000."""
        if channels is None:
            ch, n = None, (self._ds[2] if self._ds is not None else 0) if n_sel is None else int(n_sel)
        else:
            ch = np.ascontiguousarray(channels, np.int32).reshape(-1)
            n = len(ch)
        self._chk(self._L.ft8rx_ddc_stream_frames(self._h, int(m_first) & 0xFFFFFFFFFFFFFFFF, int(n_have), int(frame_len),
                                                  None if ch is None else ch.ctypes.data, n, d_audio_ptr), "ft8rx_ddc_stream_frames")

    def ddc_stream_read(self, m_first, n, want_float=False):
        """Test aid: outputs [m_first, m_first + n) of every channel out of the ring -> int16 [n_out, n] (, float32 [n_out, n])."""
        if self._ds is None:
            raise Ft8rxError("ddc_stream_read: no stream is open (ddc_stream_open)")
        y = np.zeros((self._ds[2], int(n)), np.int16)
        f = np.zeros((self._ds[2], int(n)), np.float32) if want_float else None
        self._chk(self._L.ft8rx_ddc_stream_read(self._h, int(m_first) & 0xFFFFFFFFFFFFFFFF, int(n), y.ctypes.data,
                                                f.ctypes.data if want_float else None), "ft8rx_ddc_stream_read")
        return (y, f) if want_float else y

    def ddc_stream_info(self):
        """-> {"in_capacity", "out_capacity", "n_pushed", "m_produced"}: ring capacities in samples, samples pushed, outputs produced
        (absolute index one past the last)."""
        v = [C.c_uint64() for _ in range(4)]
        self._chk(self._L.ft8rx_ddc_stream_info(self._h, *[C.byref(x) for x in v]), "ft8rx_ddc_stream_info")
        return dict(zip(("in_capacity", "out_capacity", "n_pushed", "m_produced"), (int(x.value) for x in v)))

    def ddc_stream_close(self):
        self._chk(self._L.ft8rx_ddc_stream_close(self._h), "ft8rx_ddc_stream_close")
        self._ds = None

    # ---- the spectrogram stage behind the open stream, plain or pre-stage (ft8rx_ddc_stream_grid_*)
    def ddc_stream_grid_open(self, hop_phase, n_rows=750):
        """Open the grid before the first push: row q of every channel is the spectrogram row of the 12 kHz outputs
        [hop_phase + 480 q - 3840, hop_phase + 480 q); the newest n_rows (16 .. 750) rows per channel are held on the device."""
        self._chk(self._L.ft8rx_ddc_stream_grid_open(self._h, int(hop_phase), int(n_rows)), "ft8rx_ddc_stream_grid_open")

    def ddc_stream_grid_info(self):
        """-> {"q_first_held", "q_next", "cols", "n_rows"}: the grid ring holds rows [q_first_held, q_next) of `cols` values."""
        q = [C.c_uint64(), C.c_uint64()]
        v = [C.c_int32(), C.c_int32()]
        self._chk(self._L.ft8rx_ddc_stream_grid_info(self._h, *[C.byref(x) for x in q + v]), "ft8rx_ddc_stream_grid_info")
        return dict(zip(("q_first_held", "q_next", "cols", "n_rows"), (int(x.value) for x in q + v)))

    def ddc_stream_grid_read(self, q_first, n):
        """Rows [q_first, q_first + n) of every channel -> float32 [n_out, n, grid_cols], once the stream's work is done."""
        if self._ds is None:
            raise Ft8rxError("ddc_stream_grid_read: no stream is open (ddc_stream_open)")
        rows = np.empty((self._ds[2], max(int(n), 0), self.grid_cols), np.float32)
        self._chk(self._L.ft8rx_ddc_stream_grid_read(self._h, int(q_first) & 0xFFFFFFFFFFFFFFFF, int(n), rows.ctypes.data), "ft8rx_ddc_stream_grid_read")
        return rows

    # ---- the input pre-stages, written once: `name` is "ddc_wide" or "ddc_rat", the prefix of the C entries
    # (ft8rx_<name>*) and of the methods below, and the module that packs the samples of its kinds
    def _pre_oneshot(self, name, samples, kind, rate, f_dial_hz, gain, want_float, device, d_ptr=None, n=None, d_f32_ptr=None):
        if d_ptr is None:
            a, n = _pre_module(name).pack(samples, kind)
        f = np.ascontiguousarray(f_dial_hz, np.float64).reshape(-1)
        if len(f) < 1:
            raise Ft8rxError(f"{name}: at least one f_dial_hz")
        fm = np.zeros(len(f), np.float64)
        if d_ptr is not None:                                # on the device already: the device entry, queued and not waited for
            self._chk(getattr(self._L, f"ft8rx_{name}")(self._h, int(d_ptr), int(kind), int(rate), int(n), len(f), f.ctypes.data, float(gain),
                                                        None, d_f32_ptr, fm.ctypes.data), f"ft8rx_{name}")
            return fm
        args = (int(kind), int(rate), n, len(f), f.ctypes.data, float(gain))
        if not (device or want_float or d_f32_ptr is not None):
            self._chk(getattr(self._L, f"ft8rx_{name}_host")(self._h, a.ctypes.data, *args, fm.ctypes.data), f"ft8rx_{name}_host")
            return fm
        import torch
        dev = torch.device("cuda", self.device)
        d_in = torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
        d_f32 = torch.empty((len(f), NSAMP), dtype=torch.float32, device=dev) if want_float else None
        torch.cuda.synchronize(dev)
        self._chk(getattr(self._L, f"ft8rx_{name}")(self._h, d_in.data_ptr(), *args, None, d_f32.data_ptr() if want_float else d_f32_ptr, fm.ctypes.data), f"ft8rx_{name}")
        self.sync()                                          # the tensors may go once the kernels have run
        return (fm, d_f32.cpu().numpy()) if want_float else fm

    def _pre_open(self, name, kind, rate, f_dial_hz, gain, n_origin, keep_f32):
        f = np.ascontiguousarray(f_dial_hz, np.float64).reshape(-1)
        if len(f) < 1:
            raise Ft8rxError(f"{name}_stream_open: at least one f_dial_hz")
        fm = np.zeros(len(f), np.float64)
        self._chk(getattr(self._L, f"ft8rx_{name}_stream_open")(self._h, int(kind), int(rate), len(f), f.ctypes.data, float(gain), int(n_origin),
                                                                _keep_f32(keep_f32), fm.ctypes.data), f"ft8rx_{name}_stream_open")
        setattr(self, _PRE_FIELD[name], (int(kind), len(f)))
        self._ds = (3, len(f), len(f))                       # the stage behind: one IQ float32 stream per channel
        return fm

    def _pre_stream(self, name, what):
        """the open stream of stage `name`, or the refusal of method `what`"""
        s = getattr(self, _PRE_FIELD[name])
        if s is None:
            raise Ft8rxError(f"{name}_stream_{what}: no {_PRE_WORD[name]} stream is open ({name}_stream_open)")
        return s

    def _pre_push(self, name, samples, device, d_ptr=None, n=None):
        kind = self._pre_stream(name, "push")[0]
        entry = f"ft8rx_{name}_stream_push"
        m = C.c_uint64()
        if d_ptr is not None:                                # on the device already: queued and not waited for
            self._chk(getattr(self._L, entry)(self._h, int(d_ptr), int(n), 1, C.byref(m)), entry)
            return int(m.value)
        a, n = _pre_module(name).pack(samples, kind)
        if not device:
            self._chk(getattr(self._L, entry)(self._h, a.ctypes.data, n, 0, C.byref(m)), entry)
            return int(m.value)
        import torch
        dev = torch.device("cuda", self.device)
        d_in = torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
        torch.cuda.synchronize(dev)
        self._chk(getattr(self._L, entry)(self._h, d_in.data_ptr(), n, 1, C.byref(m)), entry)
        self.sync()
        return int(m.value)

    def _pre_read_mid(self, name, k_first, n):
        v = np.zeros((self._pre_stream(name, "read_mid")[1], int(n)), np.complex64)
        self._chk(getattr(self._L, f"ft8rx_{name}_stream_read_mid")(self._h, int(k_first), int(n), v.ctypes.data), f"ft8rx_{name}_stream_read_mid")
        return v

    def _pre_close(self, name):
        self._chk(getattr(self._L, f"ft8rx_{name}_stream_close")(self._h), f"ft8rx_{name}_stream_close")
        setattr(self, _PRE_FIELD[name], None)
        self._ds = None

    # ---- wide pre-decimator (ft8rx_ddc_wide*): ONE stream at 240 kHz .. 129.6 MHz in front of the down-converter
    def ddc_wide(self, samples, kind, rate, f_dial_hz, gain=1.0, want_float=False, device=False, d_ptr=None, n=None, d_f32_ptr=None):
        """ft8rx_ddc_wide_host / ft8rx_ddc_wide: one stream of `kind` (ddc_wide.REAL_I16 .. ddc_wide.IQ_I8; forms of ddc_wide.pack) at
        `rate` Hz into len(f_dial_hz) frames in the staging buffer -> f_mixed_hz [n_out].  want_float: -> (f_mixed_hz, y float32
        [n_out, 180000]).  device / want_float: through a torch tensor and the device entry, as Handle.ddc."""
        return self._pre_oneshot("ddc_wide", samples, kind, rate, f_dial_hz, gain, want_float, device, d_ptr, n, d_f32_ptr)

    def ddc_wide_stream_open(self, kind, rate, f_dial_hz, gain=1.0, n_origin=0, keep_f32=False):
        """Open the wide stream: one input of `kind` at `rate` Hz feeds len(f_dial_hz) channels; n_origin = absolute index of the first
        sample that will be pushed, a multiple of 1008 rate / 12000.  -> f_mixed_hz.  ddc_stream_frame / _read / _info then work on it."""
        return self._pre_open("ddc_wide", kind, rate, f_dial_hz, gain, n_origin, keep_f32)

    def ddc_wide_stream_push(self, samples, device=False, d_ptr=None, n=None):
        """Push the next samples (forms of ddc_wide.pack; 1 .. one second) -> absolute index one past the last 12 kHz output produced
        so far.  Asynchronous.  device: through a torch tensor and the device form of the entry (the call then waits for the stream).
        d_ptr, n: the n next samples, on the device already (a raw address, what blank_in_stream_push releases)."""
        return self._pre_push("ddc_wide", samples, device, d_ptr, n)

    def ddc_wide_stream_read_mid(self, k_first, n):
        """Test aid: intermediate samples [k_first, k_first + n) of every channel -> complex64 [n_out, n]."""
        return self._pre_read_mid("ddc_wide", k_first, n)

    def ddc_wide_stream_close(self):
        self._pre_close("ddc_wide")

    # ---- rational resampler (ft8rx_ddc_rat*): ONE stream at 44.1 kHz, 2.048 MS/s, ... in front of the down-converter
    def ddc_rat(self, samples, kind, rate, f_dial_hz, gain=1.0, want_float=False, device=False, d_ptr=None, n=None, d_f32_ptr=None):
        """ft8rx_ddc_rat_host / ft8rx_ddc_rat: one stream of `kind` (ddc_rat.REAL_I16 .. ddc_rat.IQ_I8; forms of ddc_rat.pack) at `rate`
        Hz into len(f_dial_hz) frames in the staging buffer -> f_mixed_hz [n_out].  want_float: -> (f_mixed_hz, y float32
        [n_out, 180000]).  device / want_float: through a torch tensor and the device entry, as Handle.ddc."""
        return self._pre_oneshot("ddc_rat", samples, kind, rate, f_dial_hz, gain, want_float, device, d_ptr, n, d_f32_ptr)

    def ddc_rat_stream_open(self, kind, rate, f_dial_hz, gain=1.0, n_origin=0, keep_f32=False):
        """Open the rational stream: one input of `kind` at `rate` Hz feeds len(f_dial_hz) channels; n_origin = absolute index of the
        first sample that will be pushed (ddc_rat.origin_ok).  -> f_mixed_hz.  ddc_stream_frame / _read / _info then work on it."""
        return self._pre_open("ddc_rat", kind, rate, f_dial_hz, gain, n_origin, keep_f32)

    def ddc_rat_stream_push(self, samples, device=False, d_ptr=None, n=None):
        """Push the next samples (forms of ddc_rat.pack; 1 .. one second) -> absolute index one past the last 12 kHz output produced so
        far.  Asynchronous.  device: through a torch tensor and the device form of the entry (the call then waits for the stream).
        d_ptr, n: the n next samples, on the device already (a raw address, what blank_in_stream_push releases)."""
        return self._pre_push("ddc_rat", samples, device, d_ptr, n)

    def ddc_rat_stream_read_mid(self, k_first, n):
        """Test aid: intermediate samples [k_first, k_first + n) of every channel -> complex64 [n_out, n]."""
        return self._pre_read_mid("ddc_rat", k_first, n)

    def ddc_rat_stream_close(self):
        self._pre_close("ddc_rat")

    # ---- noise blanker (ft8rx_blank*; pyft8_amd/blanker.py holds the twin and the parameter checks)
    def blank(self, d_audio_ptr, n_frames, threshold_q8=2048, guard=6, taper=6, want_stats=True, want_levels=False):
        """ft8rx_blank: blank n_frames frames in place on the device (d_audio_ptr: a raw device pointer, None = the staging audio)
        -> stats int32 [n_frames, 4] (None without want_stats: the call is then only queued); want_levels: -> (stats, levels int32
        [n_frames, 375, 2] = (m_b, L_b))."""
        B = int(n_frames)
        stats = np.zeros((max(B, 0), 4), np.int32) if want_stats else None
        lv = np.zeros((max(B, 0), 375, 2), np.int32) if want_levels else None
        self._chk(self._L.ft8rx_blank(self._h, d_audio_ptr or None, B, int(threshold_q8), int(guard), int(taper),
                                      stats.ctypes.data if want_stats else None, lv.ctypes.data if want_levels else None), "ft8rx_blank")
        return (stats, lv) if want_levels else stats

    def blank_host(self, audio, threshold_q8=2048, guard=6, taper=6):
        """ft8rx_blank_host: host frames int16 [n_frames, 180000] -> the staging audio, blanked there (enqueue(staging_ptr(), n) is the
        next call) -> stats int32 [n_frames, 4]."""
        audio = _audio(audio, f"blank_host: audio must be int16 [n_frames, {NSAMP}], got shape {{shape}}")
        stats = np.zeros((len(audio), 4), np.int32)
        self._chk(self._L.ft8rx_blank_host(self._h, audio.ctypes.data, len(audio), int(threshold_q8), int(guard), int(taper), stats.ctypes.data),
                  "ft8rx_blank_host")
        return stats

    # ---- input-rate noise blanker (ft8rx_blank_in*; pyft8_amd/blank_in.py holds the twin and the parameter checks)
    def blank_in(self, samples, kind, block=1024, threshold_q8=None, guard=6, taper=6, d_ptr=None, n=None, d_out=None, want_stats=True,
                 want_levels=False, download=False):
        """ft8rx_blank_in_host / ft8rx_blank_in: blank ONE stream's samples of `kind` (forms of blank_in.pack) at their own rate.
        Host samples go into the handle's device buffer and are blanked there -> (d_ptr, n, stats int64 [4]): the raw device address
        a down-converter's d_ptr argument takes, valid until the next blank_in call.  d_ptr, n: samples on the device already, in
        place or into d_out -> (d_out or d_ptr, n, stats or None[, levels int32 [n_blocks, 2] = (m_b, L_b)]).  download: the blanked
        samples come back too, as the last element."""
        from . import blank_in as _bi, kinds as _k
        q8 = int(threshold_q8) if threshold_q8 is not None else int(256 * _bi.threshold_default(kind))
        stats = np.zeros(4, np.int64) if want_stats else None
        if d_ptr is None:
            a, n = _bi.pack(samples, kind)
            out = C.c_void_p()
            self._chk(self._L.ft8rx_blank_in_host(self._h, a.ctypes.data, int(kind), n, int(block), q8, int(guard), int(taper),
                                                  stats.ctypes.data if want_stats else None, C.byref(out)), "ft8rx_blank_in_host")
            res = [int(out.value or 0), n, stats]
            shape, dt = a.shape, a.dtype
        else:
            n = int(n)
            lv = np.zeros((max(-(-n // max(int(block), 1)), 0), 2), np.int32) if want_levels else None
            self._chk(self._L.ft8rx_blank_in(self._h, int(d_ptr), int(kind), n, int(block), q8, int(guard), int(taper), d_out or None,
                                             stats.ctypes.data if want_stats else None, lv.ctypes.data if want_levels else None), "ft8rx_blank_in")
            res = [int(d_out or d_ptr), n, stats] + ([lv] if want_levels else [])
            shape, dt = _k.shape(kind, n), _k.DTYPE[kind]
        if download:
            y = np.empty(shape, dt)
            self.sync()
            self._chk(self._L.ft8rx_copy_to_host(self._h, y.ctypes.data, res[0], y.nbytes), "ft8rx_copy_to_host")
            res.append(y)
        return tuple(res)

    def blank_in_stream_open(self, kind, block=1024, threshold_q8=None, guard=6, taper=6, n_origin=0, max_push=1 << 20):
        """Open the handle's input blanker stream (one per handle, independent of the down-converter streams): everything is allocated
        here and released by blank_in_stream_close."""
        from . import blank_in as _bi
        q8 = int(threshold_q8) if threshold_q8 is not None else int(256 * _bi.threshold_default(kind))
        self._chk(self._L.ft8rx_blank_in_stream_open(self._h, int(kind), int(block), q8, int(guard), int(taper), int(n_origin), int(max_push)),
                  "ft8rx_blank_in_stream_open")
        self._bis = int(kind)

    def blank_in_stream_push(self, samples=None, finish=False, d_ptr=None, n=None, download=False):
        """Push the next samples (forms of blank_in.pack, 0 .. max_push; None = none; d_ptr, n: on the device already) -> (d_out,
        n_first, n_out): the raw device address, absolute index and count of the samples this push released, valid until the next
        push.  finish: the stream ends here and everything left is released.  download: -> (d_out, n_first, n_out, samples)."""
        from . import blank_in as _bi, kinds as _k
        if getattr(self, "_bis", None) is None:
            raise Ft8rxError("blank_in_stream_push: no input blanker stream is open (blank_in_stream_open)")
        kind = self._bis
        out, first, cnt = C.c_void_p(), C.c_uint64(), C.c_uint64()
        if d_ptr is not None:
            args = (int(d_ptr), int(n), 1)
        elif samples is None:
            args = (None, 0, 0)
        else:
            a, n = _bi.pack(samples, kind)
            args = (a.ctypes.data, n, 0)
        self._chk(self._L.ft8rx_blank_in_stream_push(self._h, *args, int(bool(finish)), C.byref(out), C.byref(first), C.byref(cnt)),
                  "ft8rx_blank_in_stream_push")
        res = (int(out.value or 0), int(first.value), int(cnt.value))
        if not download:
            return res
        y = np.empty(_k.shape(kind, res[2]), _k.DTYPE[kind])
        if res[2]:
            self.sync()
            self._chk(self._L.ft8rx_copy_to_host(self._h, y.ctypes.data, res[0], y.nbytes), "ft8rx_copy_to_host")
        return res + (y,)

    def blank_in_stream_info(self):
        """-> {"n_pushed", "n_released", "stats"}: samples pushed, absolute index of the first sample not released, int64 [4]"""
        p, r = C.c_uint64(), C.c_uint64()
        stats = np.zeros(4, np.int64)
        self._chk(self._L.ft8rx_blank_in_stream_info(self._h, C.byref(p), C.byref(r), stats.ctypes.data), "ft8rx_blank_in_stream_info")
        return {"n_pushed": int(p.value), "n_released": int(r.value), "stats": stats}

    def blank_in_stream_close(self):
        self._chk(self._L.ft8rx_blank_in_stream_close(self._h), "ft8rx_blank_in_stream_close")
        self._bis = None

    # ---- panorama (ft8rx_pan*; pyft8_amd/pan.py holds the twin, the parameter checks and the axes)
    @staticmethod
    def _pan_stats(kind, stats):
        from . import kinds as _k
        return stats.astype(np.int64) if _k.is_integer(kind) else None

    def pan(self, samples, kind, n_fft=2048, n_avg=1, d_ptr=None, n=None):
        """ft8rx_pan_host / ft8rx_pan: the panorama of ONE stream's samples of `kind` (forms of pan.pack; d_ptr, n: on the device
        already) -> (rows float32 [n_rows, bins] = sums of n_avg window powers, stats int64 [n_rows, 2] = (samples at a rail, largest
        |c|), None for a float kind)."""
        from . import pan as _pan
        if d_ptr is None:
            a, n = _pan.pack(samples, kind)
            entry, name, src = self._L.ft8rx_pan_host, "ft8rx_pan_host", a.ctypes.data
        else:
            entry, name, src, n = self._L.ft8rx_pan, "ft8rx_pan", int(d_ptr), int(n)
        n_rows = max(n // max(int(n_fft), 1) // max(int(n_avg), 1), 0)
        rows = np.zeros((n_rows, _pan.bins(kind, max(int(n_fft), 2))), np.float32)
        stats = np.zeros((n_rows, 2), np.int32)
        cnt = C.c_uint64()
        self._chk(entry(self._h, src, int(kind), n, int(n_fft), int(n_avg), rows.ctypes.data, stats.ctypes.data, C.byref(cnt)), name)
        if int(cnt.value) != n_rows:
            raise Ft8rxError(f"{name}: {cnt.value} rows, expected {n_rows}")
        return rows, self._pan_stats(kind, stats)

    def pan_host(self, samples, kind, n_fft=2048, n_avg=1):
        return self.pan(samples, kind, n_fft, n_avg)

    def pan_stream_open(self, kind, n_fft=2048, n_avg=1, n_rows=256, n_origin=0, max_push=1 << 20):
        """Open the handle's panorama stream (one per handle, independent of every other stream): everything is allocated here and
        released by pan_stream_close."""
        self._chk(self._L.ft8rx_pan_stream_open(self._h, int(kind), int(n_fft), int(n_avg), int(n_rows), int(n_origin), int(max_push)),
                  "ft8rx_pan_stream_open")
        self._pans = int(kind)

    def pan_stream_push(self, samples=None, d_ptr=None, n=None):
        """Push the next samples (forms of pan.pack, 0 .. max_push; d_ptr, n: on the device already) -> (d_samples, rows_done): the raw
        device address of the chunk's first sample in the stream's work buffer, valid until the next push (what a down-converter's
        d_ptr push takes), and the first row that is not complete yet."""
        from . import pan as _pan
        if getattr(self, "_pans", None) is None:
            raise Ft8rxError("pan_stream_push: no panorama stream is open (pan_stream_open)")
        out, done = C.c_void_p(), C.c_uint64()
        if d_ptr is not None:
            args = (int(d_ptr), int(n), 1)
        elif samples is None:
            args = (None, 0, 0)
        else:
            a, n = _pan.pack(samples, self._pans)
            args = (a.ctypes.data, n, 0)
        self._chk(self._L.ft8rx_pan_stream_push(self._h, *args, C.byref(out), C.byref(done)), "ft8rx_pan_stream_push")
        return int(out.value or 0), int(done.value)

    def pan_stream_info(self):
        """-> {"n_pushed", "rows_done", "r_lo", "bins"}: samples pushed, the first row not complete, the oldest row held, bins per row"""
        p, d, lo, b = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        self._chk(self._L.ft8rx_pan_stream_info(self._h, C.byref(p), C.byref(d), C.byref(lo), C.byref(b)), "ft8rx_pan_stream_info")
        return {"n_pushed": int(p.value), "rows_done": int(d.value), "r_lo": int(lo.value), "bins": int(b.value)}

    def pan_stream_read(self, r_first, n):
        """The finished rows [r_first, r_first + n) -> (rows float32 [n, bins], stats int64 [n, 2] or None for a float kind)"""
        bins = self.pan_stream_info()["bins"]
        rows, stats = np.zeros((max(int(n), 0), bins), np.float32), np.zeros((max(int(n), 0), 2), np.int32)
        self._chk(self._L.ft8rx_pan_stream_read(self._h, int(r_first), int(n), rows.ctypes.data, stats.ctypes.data), "ft8rx_pan_stream_read")
        return rows, self._pan_stats(self._pans, stats)

    def pan_stream_close(self):
        self._chk(self._L.ft8rx_pan_stream_close(self._h), "ft8rx_pan_stream_close")
        self._pans = None

    def pinned_audio(self, n_frames):
        """int16 [n_frames, 180000] array in page-locked host memory (ft8rx_alloc_host): fill it and pass it to decode_batch for
        overlapped DMA.  The memory is released when the array (and every view of it) is garbage collected."""
        return self.pinned_bytes(int(n_frames) * NSAMP * 2).view(np.int16).reshape(int(n_frames), NSAMP)

    def staging_ptr(self):
        return int(self._L.ft8rx_staging_audio(self._h))

    def download_audio(self, d_ptr, n_frames):
        out = np.empty((n_frames, NSAMP), np.int16)
        self._chk(self._L.ft8rx_copy_to_host(self._h, out.ctypes.data, d_ptr, out.nbytes), "ft8rx_copy_to_host")
        return out

    def synth_frames(self, d_audio_ptr, start, count, n_signals=50, snr_range=(-10.0, 10.0), seed=0x4654385F53594E54, noise=True,
                     return_table=False):
        """Fill the device buffer at d_audio_ptr ([count][180000] int16) with synthetic frames; returns the truth list (and the
        signal table handed to the kernel if return_table).  noise=False leaves the Philox noise out (parity tests)."""
        from . import synth
        recs, truth = synth.device_signal_table(start, count, n_signals, snr_range)
        assert recs.dtype.itemsize == synth.SIGNAL_DTYPE.itemsize
        q = np.ascontiguousarray(synth.pulse_cumsum(), np.float64)
        self._chk(self._L.ft8rx_synth_frames_ex(self._h, int(seed), int(start), int(count), int(n_signals), recs.ctypes.data,
                                              int(recs.dtype.itemsize), q.ctypes.data, d_audio_ptr, int(not noise)), "ft8rx_synth_frames")
        return (truth, recs) if return_table else truth

    def math_probe(self, which, x):
        x = np.ascontiguousarray(x, np.complex64 if which == 2 else np.float32)          # 2: an FFT of length len(x)
        y = np.empty_like(x)
        self._chk(self._L.ft8rx_math_probe(self._h, int(which), x.ctypes.data, len(x) if which == 2 else x.size, y.ctypes.data), "ft8rx_math_probe")
        return y


PKG_MSG_TRUNCATED, PKG_EVENTS_TRUNCATED = 1, 2


class Ft8rxTruncationWarning(RuntimeWarning):
    """A frame's event log (FT8RX_EVENT_CAP) or message list overflowed: see include/ft8rx.h FT8RX_PKG_*."""


class CallHashTable:
    """Persistent native call-hash table (ft8rx_hashes_*; reference databases.py:8-26) for package_batch(table=...)."""

    def __init__(self):
        self._t = C.c_void_p(lib().ft8rx_hashes_create())
        if not self._t.value:
            raise Ft8rxError("ft8rx_hashes_create failed")

    def add(self, call):
        lib().ft8rx_hashes_add(self._t, call.encode())

    def clear(self):
        lib().ft8rx_hashes_clear(self._t)

    def __len__(self):
        return int(lib().ft8rx_hashes_size(self._t))

    def __del__(self):
        try:
            if self._t.value:
                lib().ft8rx_hashes_destroy(self._t)
                self._t = C.c_void_p()
        except Exception:
            pass


def set_reject_log(path):
    """Turn the reference's rejected_callsigns.txt side effect (decoders.py:114-115) on (path) or off (None) -- in every loaded build
    of the library (the packager inside Handle.decode_messages is the wide build's own copy on a wide handle)."""
    _reject_log[0] = path
    lib()
    for L in _libs.values():
        L.ft8rx_set_reject_log(path.encode() if path else None)


def _chk_host(rc, what):
    if rc != 0:
        raise Ft8rxError(f"{what} failed ({rc})")


def _package(who, fn, head, B, max_msgs, n_threads, table, out=None, dtype=MESSAGE_DTYPE, tail=(), chk=_chk_host):
    """What every packaging entry shares: fn(*head, out, max_msgs, out_counts, n_threads, table, flags, *tail) into fresh (messages
    [B, max_msgs] of dtype, counts [B], flags [B]) or the caller's `out`, the thread default, the return code and the truncation
    warning (raised in the name of who's caller) -> (messages, counts, flags)."""
    msgs, oc, flags = out if out is not None else (np.zeros((B, max_msgs), dtype), np.zeros(B, np.int32), np.zeros(B, np.int32))
    if n_threads is None:
        n_threads = min(32, os.cpu_count() or 1)
    chk(fn(*head, msgs.ctypes.data, int(max_msgs), oc.ctypes.data, int(n_threads), table._t if table is not None else None,
           flags.ctypes.data, *tail), fn.__name__)
    if flags.any():
        import warnings
        nev, nmsg = int((flags & PKG_EVENTS_TRUNCATED != 0).sum()), int((flags & PKG_MSG_TRUNCATED != 0).sum())
        warnings.warn(f"{who}: event log overflowed in {nev} frame(s) (> {EVENT_CAP} CRC-passing words: `<...>` strings may differ), "
                      f"message list truncated in {nmsg} frame(s)", Ft8rxTruncationWarning, stacklevel=3)
    return msgs, oc, flags


def _dense(who, rec, cnt, ev, evc, recall=None):
    """The dense result arrays as the packagers take them -> ([records, counts, events, event_counts (, recall, recall_counts)],
    n_frames, max_cands)."""
    arrs = [np.ascontiguousarray(rec), np.ascontiguousarray(cnt, np.int32), np.ascontiguousarray(ev), np.ascontiguousarray(evc, np.int32)]
    if recall is not None:
        arrs += [np.ascontiguousarray(recall[0], RECORD_DTYPE), np.ascontiguousarray(recall[1], np.int32)]
    rec, ev = arrs[0], arrs[2]
    B, mc = rec.shape
    if (ev.shape != (B, EVENT_CAP) or rec.dtype != RECORD_DTYPE or ev.dtype != EVENT_DTYPE
            or (recall is not None and (arrs[4].shape != (B, RECALL_MAX) or arrs[5].shape != (B,)))):
        what, source = ("records/events", "fetch") if recall is None else ("records/events/recall", "fetch_recall")
        raise Ft8rxError(f"{who}: {what} are not the arrays returned by decode_batch/{source}")
    return arrs, B, mc


def package_batch(rec, cnt, ev, evc, max_msgs=None, n_threads=None, table=None, return_flags=False, out=None):
    """Native host message layer (ft8rx_package_batch): records/events of B frames -> (messages[B, max_msgs], counts[B]).
    Pure host code: works without a GPU.  max_msgs defaults to the record capacity (so the list cannot be truncated); table = a
    CallHashTable shared by the frames in order (streaming) instead of a fresh table per frame.  An overflowed event log or
    message list raises Ft8rxTruncationWarning (warnings module) and is reported per frame in the flags (return_flags=True).
    out = the (messages, counts, flags) arrays of an earlier call with return_flags=True: written in place instead of fresh arrays
    (message slots beyond the counts are stale then)."""
    arrs, B, mc = _dense("package_batch", rec, cnt, ev, evc)
    if max_msgs is None:
        max_msgs = max(mc, 1)
    if out is not None:
        msgs, oc, flags = out
        if (msgs.shape != (B, max_msgs) or msgs.dtype != MESSAGE_DTYPE or oc.shape != (B,) or oc.dtype != np.int32 or flags.shape != (B,)
                or flags.dtype != np.int32 or not all(a.flags.c_contiguous and a.flags.writeable for a in (msgs, oc, flags))):
            raise Ft8rxError("package_batch: `out` does not fit this batch")
    res = _package("package_batch", lib().ft8rx_package_batch, [a.ctypes.data for a in arrs] + [int(B), int(mc)], B, max_msgs, n_threads,
                   table, out=out)
    return res if return_flags else res[:2]


def package_batch_ext(rec, cnt, ev, evc, mask, max_msgs=None, n_threads=None, table=None, return_flags=False):
    """ft8rx_package_batch_ext: package_batch for records decoded with msg_types = mask -> (messages[B, max_msgs] of
    MESSAGE_EXT_DTYPE, counts[B]).  mask = 0 renders what package_batch renders."""
    arrs, B, mc = _dense("package_batch_ext", rec, cnt, ev, evc)
    if max_msgs is None:
        max_msgs = max(mc, 1)
    res = _package("package_batch_ext", lib().ft8rx_package_batch_ext, [a.ctypes.data for a in arrs] + [int(B), int(mc)], B, max_msgs,
                   n_threads, table, dtype=MESSAGE_EXT_DTYPE, tail=(int(mask),))
    return res if return_flags else res[:2]


def package_batch_recall(rec, cnt, ev, evc, rrec, rcnt, max_msgs=None, n_threads=None, table=None):
    """ft8rx_package_batch_recall: package_batch, then each frame's accepted recall records (fetch_recall) after its ladder messages,
    in entry order, unless the frame has the text already -> (messages[B, max_msgs], counts[B])."""
    arrs, B, mc = _dense("package_batch_recall", rec, cnt, ev, evc, recall=(rrec, rcnt))
    if max_msgs is None:
        max_msgs = max(mc, 1) + RECALL_MAX
    return _package("package_batch_recall", lib().ft8rx_package_batch_recall, [a.ctypes.data for a in arrs] + [int(B), int(mc)], B, max_msgs,
                    n_threads, table)[:2]


def recall_hypotheses(entry):
    """ft8rx_recall_hypotheses (host only): the hypothesis words of one entry (RECALL_ENTRY_DTYPE) as Python ints, in list order;
    [] for an entry that does not qualify."""
    e = np.asarray(entry, RECALL_ENTRY_DTYPE).reshape(1)
    lo, hi = np.zeros(126, np.uint64), np.zeros(126, np.uint64)
    n = lib().ft8rx_recall_hypotheses(e.ctypes.data, lo.ctypes.data, hi.ctypes.data)
    if n < 0:
        raise Ft8rxError("ft8rx_recall_hypotheses failed")
    return [(int(hi[i]) << 64) | int(lo[i]) for i in range(n)]


def packed_capacity(n_frames, max_cands=MAX_CANDS, per_frame=None):
    """Bytes a packed result buffer needs for n_frames frames: the worst case (every candidate kept, full event logs) by default, or
    per_frame bytes of records + events per frame (config 1 frames use ~4 KB; an overflow is flagged, never silent)."""
    worst = RECORD_DTYPE.itemsize * int(max_cands) + EVENT_DTYPE.itemsize * EVENT_CAP
    body = worst if per_frame is None else min(worst, int(per_frame))
    return PACKED_HEADER_DTYPE.itemsize + int(n_frames) * (PACKED_FRAME_DTYPE.itemsize + body)


def pack_results(rec, cnt, ev, evc):
    """Host twin of the k_pack_* kernels: dense result arrays (as returned by fetch / decode_batch) -> one uint8 array in the packed
    layout of include/ft8rx.h.  Used where results are host arrays already (the gloo gather of tests, tools)."""
    rec = np.ascontiguousarray(rec)
    B, mc = rec.shape
    cnt = np.clip(np.asarray(cnt, np.int64), 0, mc)
    evc = np.asarray(evc, np.int64)
    nev = np.clip(evc, 0, EVENT_CAP)
    keep = np.zeros((B, mc), bool)
    for f in range(B):
        n = int(cnt[f])
        k = rec[f, :n]["status"] == ST_DECODED
        c = np.asarray(ev[f, :int(nev[f])]["cand"], np.int64)
        k[c[c < n]] = True
        if np.isnan(rec[f, :n]["grid_sd"]).any() or np.isnan(rec[f, :n]["fine_sd"]).any():
            k[:] = True
        keep[f, :n] = k
    nrec = keep.sum(1)
    table = np.zeros(B, PACKED_FRAME_DTYPE)
    table["rec_off"] = np.concatenate([[0], np.cumsum(nrec)[:-1]]) if B else []
    table["ev_off"] = np.concatenate([[0], np.cumsum(nev)[:-1]]) if B else []
    table["n_cand"], table["n_rec"], table["n_ev"] = cnt, nrec, np.maximum(evc, 0)
    recs = rec[keep].copy()                                   # row-major boolean take: frame order, candidate order inside a frame
    recs["pad2"] = np.nonzero(keep)[1]
    evs = np.concatenate([ev[f, :int(nev[f])] for f in range(B)]) if B else np.zeros(0, EVENT_DTYPE)
    hdr = np.zeros(1, PACKED_HEADER_DTYPE)
    hdr["magic"], hdr["n_frames"], hdr["n_records"], hdr["n_events"], hdr["max_cands"] = PACKED_MAGIC, B, len(recs), len(evs), mc
    hdr["bytes"] = hdr.nbytes + table.nbytes + recs.nbytes + evs.nbytes
    return np.concatenate([hdr.view(np.uint8), table.view(np.uint8), recs.view(np.uint8).reshape(-1), evs.view(np.uint8).reshape(-1)])


class Packed:
    """Read-only view of a packed result buffer (any object with the buffer protocol; nothing is copied): .header, .frames (the
    frame table), .records, .events, frame(f) -> (records, events) of one frame."""

    def __init__(self, buf):
        b = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf.view(np.uint8).reshape(-1)
        if b.size < PACKED_HEADER_DTYPE.itemsize:
            raise Ft8rxError("packed results: buffer shorter than a header")
        self.header = b[:32].view(PACKED_HEADER_DTYPE)[0]
        h = self.header
        if int(h["magic"]) != PACKED_MAGIC:
            raise Ft8rxError("packed results: bad magic")
        if int(h["overflow"]):
            raise Ft8rxError(f"packed results: {int(h['bytes'])} bytes did not fit the buffer handed to set_packed_output")
        nf, nr, ne = int(h["n_frames"]), int(h["n_records"]), int(h["n_events"])
        o1 = 32 + 16 * nf
        o2 = o1 + RECORD_DTYPE.itemsize * nr
        o3 = o2 + EVENT_DTYPE.itemsize * ne
        if o3 != int(h["bytes"]) or o3 > b.size:
            raise Ft8rxError("packed results: inconsistent sizes")
        self.nbytes = o3
        self.buf = b[:o3]
        self.n_frames, self.max_cands = nf, int(h["max_cands"])
        self.frames = b[32:o1].view(PACKED_FRAME_DTYPE)
        self.records = b[o1:o2].view(RECORD_DTYPE)
        self.events = b[o2:o3].view(EVENT_DTYPE)

    def frame(self, f):
        t = self.frames[f]
        return (self.records[int(t["rec_off"]):int(t["rec_off"]) + int(t["n_rec"])],
                self.events[int(t["ev_off"]):int(t["ev_off"]) + min(int(t["n_ev"]), EVENT_CAP)])

    def expand(self):
        """-> dense (records[B, max_cands], counts[B], events[B, EVENT_CAP], event_counts[B]) with the kept records at their candidate
        positions; every other record is zero (tests, tools)."""
        B, mc = self.n_frames, self.max_cands
        rec = np.zeros((B, mc), RECORD_DTYPE)
        ev = np.zeros((B, EVENT_CAP), EVENT_DTYPE)
        for f in range(B):
            r, e = self.frame(f)
            idx = r["pad2"].astype(np.int64)
            rr = r.copy()
            rr["pad2"] = 0
            rec[f, idx] = rr
            ev[f, :len(e)] = e
        return rec, self.frames["n_cand"].astype(np.int32), ev, self.frames["n_ev"].astype(np.int32)


def package_packed(buf, frame_lo=0, n_frames=None, max_msgs=None, n_threads=None, table=None, return_flags=False):
    """ft8rx_package_packed (host only): the messages of frames [frame_lo, frame_lo + n_frames) of a packed result buffer, as
    package_batch renders them from the dense arrays."""
    pk = buf if isinstance(buf, Packed) else Packed(buf)
    n = pk.n_frames - frame_lo if n_frames is None else int(n_frames)
    if max_msgs is None:
        max_msgs = max(pk.max_cands, 1)
    if n > 0:
        res = _package("package_packed", lib().ft8rx_package_packed, [pk.buf.ctypes.data, pk.nbytes, int(frame_lo), n], n, max_msgs,
                       n_threads or None, table)
    else:
        res = (np.zeros((0, max_msgs), MESSAGE_DTYPE), np.zeros(0, np.int32), np.zeros(0, np.int32))
    return res if return_flags else res[:2]


def merge_messages(out, out_counts, add, add_counts, pass_tag, drop_osd=False):
    """ft8rx_merge_messages: append (in place) the messages of a later pass that are new for their frame; -> (fresh, fresh_counts),
    the appended messages without the pass tag."""
    if out.dtype != MESSAGE_DTYPE or add.dtype != MESSAGE_DTYPE or not out.flags.c_contiguous or out.shape[0] != add.shape[0]:
        raise Ft8rxError("merge_messages: message arrays as returned by package_batch expected")
    add = np.ascontiguousarray(add)
    add_counts = np.ascontiguousarray(add_counts, np.int32)
    if out_counts.dtype != np.int32 or not out_counts.flags.c_contiguous:
        raise Ft8rxError("merge_messages: out_counts must be a contiguous int32 array (it is updated in place)")
    fresh = np.zeros_like(add)
    fc = np.zeros(add.shape[0], np.int32)
    _chk_host(lib().ft8rx_merge_messages(out.ctypes.data, out_counts.ctypes.data, int(out.shape[1]), add.ctypes.data, add_counts.ctypes.data,
                                         int(add.shape[1]), int(out.shape[0]), int(pass_tag), int(bool(drop_osd)), fresh.ctypes.data,
                                         fc.ctypes.data), "ft8rx_merge_messages")
    return fresh, fc


def subtraction_list(msgs, mcnt, rec, min_snr):
    """ft8rx_subtraction_list (host only): the signals a subtraction sweep removes -- every message with snr > min_snr, in emit order,
    as (tones, fHz, tsec).  -> (signals[B, max] of SUBSIG_DTYPE, counts[B])."""
    import math
    msgs = np.ascontiguousarray(msgs)
    rec = np.ascontiguousarray(rec)
    mcnt = np.ascontiguousarray(mcnt, np.int32)
    if msgs.dtype != MESSAGE_DTYPE or rec.dtype != RECORD_DTYPE or msgs.shape[0] != rec.shape[0]:
        raise Ft8rxError("subtraction_list: message / record arrays as returned by package_batch / decode_batch expected")
    B = msgs.shape[0]
    cap = max(1, int(mcnt.max()) if B else 1)
    arr = np.zeros((B, cap), SUBSIG_DTYPE)
    cnt = np.zeros(B, np.int32)
    most = lib().ft8rx_subtraction_list(msgs.ctypes.data, mcnt.ctypes.data, int(msgs.shape[1]), rec.ctypes.data, int(rec.shape[1]), int(B),
                                    int(math.floor(min_snr)), arr.ctypes.data, int(cap), cnt.ctypes.data)
    if most < 0:
        raise Ft8rxError(f"ft8rx_subtraction_list failed ({most})")
    return np.ascontiguousarray(arr[:, :max(1, most)]), cnt


_default = {}


def encode_tones(msg_lo, msg_hi):
    """77-bit words (as returned in records) -> uint8 [n, 79] tone sequences (ft8rx_encode_tones, host only)."""
    lo = np.ascontiguousarray(msg_lo, np.uint64).ravel()
    hi = np.ascontiguousarray(msg_hi, np.uint64).ravel()
    out = np.zeros((len(lo), 79), np.uint8)
    if lib().ft8rx_encode_tones(lo.ctypes.data, hi.ctypes.data, len(lo), out.ctypes.data) != 0:
        raise Ft8rxError("ft8rx_encode_tones failed")
    return out


def ft4_encode_tones(msg_lo, msg_hi):
    """77-bit words -> uint8 [n, 105] FT4 tone sequences (ft8rx_ft4_encode_tones, host only; ft4.tones105 is its twin)."""
    lo = np.ascontiguousarray(msg_lo, np.uint64).ravel()
    hi = np.ascontiguousarray(msg_hi, np.uint64).ravel()
    out = np.zeros((len(lo), 105), np.uint8)
    if lib().ft8rx_ft4_encode_tones(lo.ctypes.data, hi.ctypes.data, len(lo), out.ctypes.data) != 0:
        raise Ft8rxError("ft8rx_ft4_encode_tones failed")
    return out


def ft4_subtraction_list(rec, cnt, have=None):
    """ft8rx_ft4_subtraction_list (host only): per frame the decoded FT4 records in emit order, every word once, without the words
    of have[f] (an iterable of 77-bit integers per frame) -> (signals [B, max] of FT4_SUBSIG_DTYPE, counts [B])."""
    rec = np.ascontiguousarray(rec)
    cnt = np.ascontiguousarray(cnt, np.int32)
    if rec.dtype != RECORD_DTYPE or rec.ndim != 2 or len(cnt) != len(rec):
        raise Ft8rxError("ft4_subtraction_list: record arrays as returned by ft4_decode expected")
    B, mc = rec.shape
    hl = hh = hc = None
    mh = 0
    if have is not None:
        have = [[int(w) for w in hv] for hv in have]
        mh = max(1, max((len(hv) for hv in have), default=1))
        hl, hh, hc = np.zeros((B, mh), np.uint64), np.zeros((B, mh), np.uint64), np.zeros(B, np.int32)
        for f, hv in enumerate(have):
            hc[f] = len(hv)
            for j, w in enumerate(hv):
                hl[f, j], hh[f, j] = w & 0xFFFFFFFFFFFFFFFF, w >> 64
    cap = max(1, int(min(cnt.max(), mc)) if B else 1)
    arr = np.zeros((B, cap), FT4_SUBSIG_DTYPE)
    out = np.zeros(B, np.int32)
    most = lib().ft8rx_ft4_subtraction_list(rec.ctypes.data, cnt.ctypes.data, int(mc), int(B), hl.ctypes.data if mh else None,
                                            hh.ctypes.data if mh else None, hc.ctypes.data if mh else None, int(mh), arr.ctypes.data, int(cap),
                                            out.ctypes.data)
    if most < 0:
        raise Ft8rxError(f"ft8rx_ft4_subtraction_list failed ({most})")
    return np.ascontiguousarray(arr[:, :max(1, most)]), out


def ap_patterns(my_call=None, dx_call=None):
    """ft8rx_ap_patterns (host only): the ipass-7 patterns ap 5..10 -> (bits[6, 174], mask[6, 174]) uint8 in LLR order; raises
    Ft8rxError naming the argument for a call that is not a standard callsign."""
    L = lib()
    bits, mask = np.zeros((6, 174), np.uint8), np.zeros((6, 174), np.uint8)
    if L.ft8rx_ap_patterns((my_call or "").encode(), (dx_call or "").encode(), bits.ctypes.data, mask.ctypes.data) != 0:
        raise Ft8rxError(L.ft8rx_last_error(None).decode())
    return bits, mask


def blank_taper(taper):
    """ft8rx_blank_taper (host only): T[1 .. taper] of the noise blanker's gate, int32 [taper]"""
    w = np.zeros(max(int(taper), 1), np.int32)
    n = lib().ft8rx_blank_taper(int(taper), w.ctypes.data, len(w))
    if n < 0:
        raise Ft8rxError(f"ft8rx_blank_taper: taper {taper} outside [0, 64]")
    return w[:n]


def default_handle(max_frames=1):
    """Process-wide handle used by the function-style API in decoders.py."""
    h = _default.get("h")
    if h is None or h.max_frames < max_frames:
        if h is not None:
            h.close()
        h = Handle(max_frames=max_frames)
        _default["h"] = h
    return h
