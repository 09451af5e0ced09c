"""Live input wider than a 12 kHz frame: real or IQ samples at 12 .. 192 kHz, in chunks of any length, feed K
channels of one receiver through the streaming down-converter (ft8rx_ddc_stream_*); ONE stream at a wide rate (240 kHz .. 129.6 MHz,
8- or 16-bit integers: ddc_wide.py, section 16.2) goes through the pre-decimator in front of it (ft8rx_ddc_wide_stream_*), and with
resample=True ONE stream at any other rate ddc_rat.py takes (44.1 kHz, 2.048 MS/s: section 16.3) through the rational resampler
(ft8rx_ddc_rat_stream_*).  WideIn is the sibling of receiver.AudioIn: its
push(chunk) is what AudioIn._callback is for 12 kHz hops; Receiver.poll() runs the passes it has found due.

Time is the sample clock: the first sample is t_first, absolute 12 kHz output m is t_first + m / 12000, cycle c starts at output
m_c = round((15 c - t_first) 12000).  Drift of the source's clock against wall time is not corrected.  PassScheduler and produced()
are pure Python (tests/test_ddc_stream.py runs them without a GPU)."""
import threading as _threading

import numpy as np

from . import _lib
from . import ddc as _ddc
from . import ddc_wide as _dw
from . import ddc_rat as _dr
from . import blank_in as _bi
from . import pan as _pan
from . import kinds as _kinds

NSAMP = _lib.NSAMP
HOP = 480                     # 12 kHz samples per hop of early_decode_hops
TILE = 1008                   # outputs per tile of the down-converter (csrc/kernels/ddc.hpp: DDC_TO)
T_CYC = 15
HEAD_MAX = 6000               # a cycle is decoded if at most this many of its first outputs lie before the stream (0.5 s, taken as zero)


_ONE_STREAM = {_dw: "wide", _dr: "resampled"}         # the rates that take ONE stream through a pre-stage, in messages


def front_end(rate, resample):
    """The module of the path a rate takes: ddc for the rates of ddc.RATES (12 .. 192 kHz); ddc_wide for a wide rate (ddc_wide.plan:
    ONE stream through the pre-decimator); with `resample` ddc_rat for any other rate it accepts (ONE stream
    through the rational resampler, section 16.3), and a rate none of the three takes is refused here.  Without `resample` every
    other rate is ddc's, which refuses it as it always did."""
    if rate not in _ddc.RATES:
        if _dw.accepts(rate):
            return _dw
        if resample:
            if not _dr.accepts(rate):
                raise _lib.Ft8rxError(f"rate {rate} is taken by none of ddc, ddc_wide and ddc_rat")
            return _dr
    return _ddc


def one_stream(mod, a, iq, rate):
    """The samples of a pre-stage rate (mod: ddc_wide or ddc_rat) as ONE stream: [1][n(, 2)] -> [n(, 2)]; more streams are refused"""
    if a.ndim == (2 if a.dtype.kind == "c" else 3 if iq else 2):
        if a.shape[0] != 1:
            raise _lib.Ft8rxError(f"samples: {a.shape[0]} streams at {rate} Hz -- a {_ONE_STREAM[mod]} rate takes one stream")
        a = a[0]
    return a


def stream_zero(mod, src):
    """... and every channel reads that stream"""
    if any(int(j) != 0 for j in src):
        raise _lib.Ft8rxError(f"src: {list(src)} -- a {_ONE_STREAM[mod]} rate takes one stream, every channel reads stream 0")


def pack(samples, iq, rate, mod, kind=None):
    """The samples of any front end (mod = front_end(rate, ...)) as its Handle methods take them -> (packed [n_streams][n(, 2)], kind,
    n_streams, n).  kind: the kind a stream began with (WideIn), or None = the samples' own by mod.kind_of, complex ones without iq
    refused.  A pre-stage rate takes ONE stream (one_stream), which comes back as [1][n(, 2)]."""
    a = np.asarray(samples)
    if kind is None:
        kind = mod.kind_of(a, iq)
        if mod.is_iq(kind) and not iq:
            raise _lib.Ft8rxError("samples are complex: pass iq=True")
    if mod not in _ONE_STREAM:
        arr, n_streams, n = mod.pack(a, kind)
        return arr, kind, n_streams, n
    arr, n = mod.pack(one_stream(mod, a, iq, rate), kind)
    return arr[None], kind, 1, n


def sources(mod, src, n_streams, n_channels):
    """src, the stream each channel reads: given, one index per channel (all 0 at a pre-stage rate); None = stream 0 for every channel,
    or stream j for channel j when there are as many streams as channels"""
    if src is None:
        if n_streams != 1 and n_streams != n_channels:
            raise _lib.Ft8rxError(f"src: {n_streams} streams and {n_channels} channels -- say which stream each channel reads")
        return [0] * n_channels if n_streams == 1 else list(range(n_channels))
    if len(src) != n_channels:
        raise _lib.Ft8rxError(f"src: one stream index per channel ({n_channels}), got {len(src)}")
    if mod in _ONE_STREAM:
        stream_zero(mod, src)
    return src


def _given(**kw):
    """The keyword arguments that are set: a call without float frames is the call it always was"""
    return {k: v for k, v in kw.items() if v}


def _pre_stage(name):
    """The row of a pre-stage in HANDLE_CALLS: its Handle methods take ONE stream as [n(, 2)], and neither n_streams nor src"""
    return (lambda h, a, kind, rate, src, dials, d_f32=None: getattr(h, name)(a[0], kind, rate, dials, **_given(d_f32_ptr=d_f32)),
            lambda h, kind, rate, n_streams, src, dials, keep_f32=False: getattr(h, name + "_stream_open")(kind, rate, dials, **_given(keep_f32=keep_f32)),
            lambda h, a: getattr(h, name + "_stream_push")(a[0]),
            lambda h, d_ptr, n, kind, rate, src, dials, d_f32=None: getattr(h, name)(None, kind, rate, dials, d_ptr=d_ptr, n=n, **_given(d_f32_ptr=d_f32)),
            lambda h, d_ptr, n: getattr(h, name + "_stream_push")(None, d_ptr=d_ptr, n=n))


# module -> how the one-shot call (h, packed, kind, rate, src, dials), the stream open (h, kind, rate, n_streams, src, dials)
# and the stream push (h, packed) reach the Handle; packed is what pack() returns, [n_streams][n(, 2)].  Behind the input blanker
# (input_blanker=) the one stream is on the device already: the one-shot call (h, d_ptr, n, kind, rate, src,
# dials) and the push (h, d_ptr, n).  Float frames: the one-shot calls take d_f32, the device address that receives
# the audio before rounding, and the open takes keep_f32 (2 = the stream runs float frames)
HANDLE_CALLS = {
    _ddc: (lambda h, a, kind, rate, src, dials, d_f32=None: h.ddc(a, kind, rate, src, dials, **_given(d_f32_ptr=d_f32)),
           lambda h, kind, rate, n_streams, src, dials, keep_f32=False: h.ddc_stream_open(kind, rate, n_streams, src, dials, **_given(keep_f32=keep_f32)),
           lambda h, a: h.ddc_stream_push(a),
           lambda h, d_ptr, n, kind, rate, src, dials, d_f32=None: h.ddc(None, kind, rate, src, dials, d_ptr=d_ptr, n=n, **_given(d_f32_ptr=d_f32)),
           lambda h, d_ptr, n: h.ddc_stream_push(None, d_ptr=d_ptr, n=n)),
    _dw: _pre_stage("ddc_wide"),
    _dr: _pre_stage("ddc_rat")}


def input_blanker_params(input_blanker, kind, n_streams, rate):
    """input_blanker= of decode_stream / WideIn for a source of `kind` and n_streams -> None (off) or (block, threshold_q8, guard,
    taper); more than one stream and float / complex samples are refused, naming the keyword and the reason"""
    if input_blanker is None or input_blanker is False:
        return None
    if n_streams != 1:
        raise _lib.Ft8rxError(f"input_blanker: {n_streams} streams -- the input blanker takes one stream")
    if kind not in _bi.KINDS:
        raise _lib.Ft8rxError("input_blanker: float / complex samples -- the input blanker takes the integer kinds only (int16, uint8, int8)")
    return _bi.params(input_blanker, kind, rate)


def _last_input(D):
    """Offset of the last input a tile needs from the input of its first output (csrc/ddc_ring.hpp: last)"""
    r2 = 1 if D == 1 else 2
    r1 = D // r2
    c1 = {4: 8, 8: 15, 16: 30}.get(D, 0)
    c2 = 71 if D == 1 else 141
    return ((TILE - 1) * r2 + c2) * r1 + c1


def produced(n_pushed, D):
    """Outputs that exist after n_pushed samples of a stream that began at index 0: whole tiles whose last input has arrived
    (csrc/ddc_ring.hpp: tiles_done).  An output exists at most one tile (84 ms) + the filters' reach (about 6 ms) after its sample."""
    have = int(n_pushed) - 1 - _last_input(D)
    return 0 if have < 0 else (have // (TILE * D) + 1) * TILE


class PassScheduler:
    """Which decode passes are due, from the sample clock alone.  A pass is (cycle c, hop, m_first, n_have): hop = the hops of the
    cycle received (an early pass; n_have = 480 hop) or 0 (the complete cycle, n_have = 180000); m_first = m_c, the cycle's first
    output, which may be negative by up to 6000 for the first cycle (those outputs are zero).  Passes come in the order they fall
    due: the early hops of a cycle ascending, then the cycle itself, then the next cycle.
    The slot geometry is a parameter: period_s seconds and n_samp outputs per cycle, hop_len outputs per hop;
    the defaults are FT8's 15 s, 180000 and 480.  ft4_scheduler() is FT4's: 7.5 s, 90000, early passes given in samples."""

    def __init__(self, t_first, early_hops=(), period_s=T_CYC, n_samp=NSAMP, hop_len=HOP):
        self.t_first = float(t_first)
        self.period_s, self.n_samp, self.hop_len = period_s, int(n_samp), int(hop_len)
        self.hops = tuple(sorted(int(x) for x in early_hops))
        c = int(np.floor(self.t_first / period_s))
        while self.cycle_start(c) < -HEAD_MAX:
            c += 1
        self.cycle, self.step = c, 0                    # the next pass: hop self.hops[step], or the complete cycle at step == len(hops)

    def cycle_start(self, c):
        """m_c: the absolute output index at which cycle c (t = 15 c; period_s c) starts"""
        return int(round((self.period_s * c - self.t_first) * 12000.0))

    def due(self, m_produced):
        """The passes whose outputs all exist now (m_first + n_have <= m_produced), each handed out once"""
        out = []
        while True:
            m_c = self.cycle_start(self.cycle)
            hop = self.hops[self.step] if self.step < len(self.hops) else 0
            n_have = self.hop_len * hop if hop else self.n_samp
            if m_c + n_have > m_produced:
                return out
            out.append((self.cycle, hop, m_c, n_have))
            self.step += 1
            if not hop:
                self.cycle, self.step = self.cycle + 1, 0


# ---- per-channel modes (modes=): a channel of the live stream is an FT8 or an FT4 channel
FT8, FT4 = MODES = ("FT8", "FT4")
FT4_T_SLOT = 7.5
FT4_NSAMP = _lib.FT4_NSAMP
FT4_EARLY_S_DEFAULT = (6.0,)      # one early pass per slot: the nominal end of an FT4 signal is 5.54 s, the early rule admits +0.45 s


def ft4_scheduler(t_first, early_samples=()):
    """FT4's PassScheduler: slot c starts at m_c = round((7.5 c - t_first) 12000), its passes are (c, n, m_c, n) for every n of
    early_samples (ascending) and then the complete slot (c, 0, m_c, 90000); the first slot is the first whose start lies at most
    HEAD_MAX outputs before the stream's origin"""
    return PassScheduler(t_first, early_samples, period_s=FT4_T_SLOT, n_samp=FT4_NSAMP, hop_len=1)


def ft4_early_samples(ft4_early_decode_s):
    """ft4_early_decode_s= of Receiver -> the early passes of an FT4 slot in samples, ascending: seconds into the slot inside (0, 7.5)
    that are a whole number of 12 kHz samples; () / None = no early pass; anything else is refused by name"""
    if ft4_early_decode_s is None:
        return ()
    vals = ft4_early_decode_s if isinstance(ft4_early_decode_s, (tuple, list)) else (ft4_early_decode_s,)
    out = set()
    for v in vals:
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 < float(v) < FT4_T_SLOT:
            raise _lib.Ft8rxError(f"ft4_early_decode_s: {v!r} outside (0, 7.5) s (seconds into the slot; () = only the complete slot)")
        n = float(v) * 12000.0
        if abs(n - round(n)) > 1e-6:
            raise _lib.Ft8rxError(f"ft4_early_decode_s: {v!r} s is not a whole number of 12 kHz samples")
        out.add(int(round(n)))
    return tuple(sorted(out))


def channel_modes(modes, n_channels):
    """modes= of Receiver / start / WideIn -> None (every channel FT8: the path without the keyword) or a tuple of "FT8" / "FT4", one
    per channel.  None, one name for every channel, or a sequence with one name per channel; a wrong length or an unknown name is
    refused by name"""
    if modes is None:
        return None
    names = [modes] * n_channels if isinstance(modes, str) else list(modes)
    if len(names) != n_channels:
        raise _lib.Ft8rxError(f"modes: one per channel ({n_channels}), got {len(names)}")
    for m in names:
        if m not in MODES:
            raise _lib.Ft8rxError(f"modes: unknown mode {m!r} (\"FT8\" or \"FT4\")")
    return None if all(m == FT8 for m in names) else tuple(names)


def merge_due(due_by_mode):
    """The passes several schedulers on one clock hand out at the same moment, {mode: [(c, hop, m_first, n_have), ...]} -> one list of
    (c, hop, m_first, n_have, mode) in the order they fall due: m_first + n_have ascending, FT8 before FT4 at a tie"""
    out = [p + (mode,) for mode, due in due_by_mode.items() for p in due]
    return sorted(out, key=lambda p: (p[2] + p[3], MODES.index(p[4])))


# ---- the waterfall / search grid of the channels (waterfall=True).  The device computes row q of every channel
# from the outputs [p0 + 480 q - 3840, p0 + 480 q) (ft8rx_ddc_stream_grid_*); these pure functions say which q that is for a hop of a
# cycle, and where it goes in the 750-row grid Receiver.search reads.  The stream of a WideIn begins at output index 0.
HOPS_PER_CYCLE = NSAMP // HOP      # 375
GRID_ROWS = 2 * HOPS_PER_CYCLE     # 750: two cycles, the reference's grid


def grid_phase(m_c0):
    """p0, the hop phase of the grid: the first cycle's start m_c0 (it may be negative) modulo a hop, so that every hop of that cycle
    -- and of every later one, 375 hops apart -- ends on a row"""
    return int(m_c0) % HOP


def grid_hops_done(m_produced, p0):
    """The first row that does not exist yet when the outputs [.., m_produced) do: the number of q >= 0 with p0 + 480 q <= m_produced
    (csrc/ddc_grid_ring.hpp: hops_done)"""
    return 0 if m_produced < p0 else (int(m_produced) - p0) // HOP + 1


def grid_rows_completed(m_before, m_after, p0, n_rows=GRID_ROWS):
    """The rows [q_first, q_end) a push completes that moved m_produced from m_before to m_after, for a stream that began at output
    0: hop 0 is no row when p0 = 0 (its window holds nothing of the stream), and of more than n_rows new rows only the newest n_rows
    are held (csrc/ddc_grid_ring.hpp: completed)"""
    q_end = grid_hops_done(m_after, p0)
    q_first = max(grid_hops_done(m_before, p0), grid_hops_done(0, p0), q_end - n_rows)
    return min(q_first, q_end), q_end


def grid_place(q, m_c0, c0):
    """Row q of the device -> (cycle c, hop h in 1 .. 375, row of the 750-row grid): with q_0 = (m_c0 - p0) / 480, the row that ends
    where the first cycle c0 starts, row q is hop h = (q - q_0 - 1) mod 375 + 1 of cycle c = c0 + (q - q_0 - 1) div 375 and goes to
    grid row (375 (c mod 2) + h) mod 750 -- the odd cycle's hop 375 to row 0, the layout Receiver.search reads."""
    k = int(q) - (int(m_c0) - grid_phase(m_c0)) // HOP - 1
    c, h = int(c0) + k // HOPS_PER_CYCLE, k % HOPS_PER_CYCLE + 1
    return c, h, (HOPS_PER_CYCLE * (c % 2) + h) % GRID_ROWS


def grid_row_of(c, h, m_c0, c0):
    """The inverse: the device's row q of hop h of cycle c"""
    return (int(m_c0) - grid_phase(m_c0)) // HOP + HOPS_PER_CYCLE * (int(c) - int(c0)) + int(h)


class WideIn:
    """The wide live input of one Receiver: K = len(dial_offsets_hz) channels out of the source's streams.

    waterfall=True: the device also computes the spectrogram row of every channel at every hop, straight
    from the down-converter's output ring (ft8rx_ddc_stream_grid_*), and after every push the rows it completed are read once into
    search_grid[j] ([750][width] float32, 1.0 until written; width = the 12 kHz path's for the receiver's search_freq_range), of which
    waterfall_data[j]["data"] is a live view (the keys of AudioIn.waterfall_data).  The grid opens at the hop phase p0 = m_c mod 480
    of the scheduler's first cycle; cycle starts are 180000 = 375 x 480 outputs apart, so hop h of cycle c lands in grid row
    (375 (c mod 2) + h) mod 750 and is hop h of the very frame the complete pass decodes.  If a later cycle_start lands one sample
    off through float rounding, the grid keeps its phase.  The grid shows the audio before noise_blanker (section 17) but behind input_blanker (section 17.1),
    which works in front of the down-converter: with it the rows are those of the blanked input.  Off (the default) nothing of it exists.

    panorama=True | {"n_fft", "n_avg" or "period_s", "rows"}: the device also keeps the averaged power
    spectrum of the ONE raw stream at its own rate (ft8rx_pan_stream_*), behind input_blanker when that is on -- what the front end
    sees.  After every push the rows it finished are read once into panorama["data"] (float32 [rows, bins], row r at r mod rows, zero
    until written); panorama["stats"] holds their (samples at a rail, largest |c|), None for float samples; "r_next" is the first row
    not there yet, "f_hz" the bins' frequencies, "row_seconds" a row's length; panorama_time(r) is the time of row r's first sample.
    Without input_blanker the chunk goes to the device once, into the panorama's buffer, and the front end reads it there.

    push(chunk) takes the next samples in the forms of Receiver.decode_stream -- real int16 or float [n], complex [n] or int16 (I, Q)
    pairs [n, 2] with iq=True, several streams as [n_streams, n(, 2)] -- of any length, hands them to the down-converter on the
    receiver's live handle (created with max_frames = K) and notes the passes that have fallen due; Receiver.poll() gathers and decodes
    them.  The samples never come back to the host.  open(source) feeds push from an iterator of chunks on a daemon thread; at the
    end of a finite source it pushes zeros until the outputs of the last real sample exist, notes the passes then due and sets
    source_exhausted."""

    def __init__(self, receiver, sample_rate, iq=False, dial_offsets_hz=(0.0,), bands=None, t_first=None, src=None, resample=False,
                 waterfall=False, input_blanker=None, float_frames=False, panorama=None, modes=None):
        self._rx = receiver
        # float_frames: the stream keeps the float32 output ring (1.44 MB per channel), every pass gathers and
        # decodes float frames, and with waterfall=True the rows come from that ring
        self.float_frames = bool(float_frames)
        self.sample_rate = int(sample_rate)
        # input_blanker: the ONE stream's integer samples are blanked at their own rate on the device
        # (ft8rx_blank_in_stream_*) and what that releases goes to the front end's device push; the kind decides at the first chunk
        self.input_blanker = input_blanker
        _bi.params(input_blanker, _bi.WIDE_IQ_I16, self.sample_rate)    # a value outside the definition is refused here
        self._ib = None                                                 # (block, threshold_q8, guard, taper) once the stream is open
        self._ib_done = False                                           # flush has finished it
        # panorama: the keyword as given, refused here when outside the definition; the stream opens with the
        # first chunk, which decides the kind
        self._pan_opt = panorama
        self._pan = _pan.params(panorama, self.sample_rate)             # (n_fft, n_avg, rows) or None
        self.panorama = None
        # the path (front_end): ddc, or ONE stream through a pre-stage (ft8rx_ddc_wide_stream_* / ft8rx_ddc_rat_stream_*).  At a resampled
        # rate sample_rate / 12000 is no integer, so input counts become output counts by exact integer arithmetic at every rate (_outputs)
        self.mod = front_end(self.sample_rate, resample)
        self.wide, self.rat = self.mod is _dw, self.mod is _dr          # descriptions: pack() and HANDLE_CALLS[self.mod] are what act
        if self.mod is _ddc:
            _ddc.decimation(self.sample_rate)                           # a rate that front_end left to ddc and that ddc does not take
        self.iq = bool(iq)
        self.dials = [float(f) for f in dial_offsets_hz]
        self.n_channels = len(self.dials)
        if self.n_channels < 1:
            raise _lib.Ft8rxError("dial_offsets_hz: at least one channel")
        if bands is not None and len(bands) != self.n_channels:
            raise _lib.Ft8rxError(f"bands: one per channel ({self.n_channels}), got {len(bands)}")
        if src is not None and len(src) != self.n_channels:
            raise _lib.Ft8rxError(f"src: one stream index per channel ({self.n_channels}), got {len(src)}")
        self.bands = list(bands) if bands is not None else None
        # modes: None = every channel is an FT8 channel and nothing below differs from a receiver without the
        # keyword; else one name per channel, the channels of each mode present, one scheduler per mode (scheds, set with the clock)
        self.modes = channel_modes(modes, self.n_channels)
        self.channels = None if self.modes is None else {m: [j for j, x in enumerate(self.modes) if x == m] for m in MODES if m in self.modes}
        self.scheds = None
        self.src = None if src is None else [int(s) for s in src]
        self.t_first = t_first
        self.kind = None
        self.n_streams = None
        self.f_mixed_hz = None
        self.sched = None
        self.n_pushed = 0                        # real samples per stream
        self.m_produced = 0
        self.source_exhausted = False
        self._ready = []                         # passes that are due and not yet decoded: (cycle, hop, m_first, n_have); modes: (..., mode)
        self._lock = _threading.Lock()           # push may run on the feeder thread, poll() on the manage_cycle stand-in
        self._feeder = None
        # per channel: the texts delivered per cycle (duplicate filter) and the complete-frame messages per cycle (recall)
        self.seen = [{} for _ in range(self.n_channels)]
        self.recall_hist = [{} for _ in range(self.n_channels)]
        # waterfall=True: per channel the 750-row grid and the reference's waterfall dict on it (a live view); None otherwise
        self.waterfall = bool(waterfall)
        self.search_grid = self.waterfall_data = None
        self.grid_phase = None                   # p0, and the first cycle (c0, m_c0) the rows are placed by; the next row to read
        self._grid_c0 = self._grid_q = None
        self._spec_cache = (None, None, None)    # cycle_spectrum: (cycle, its frames [K][180000], {channel: spectrum})
        if self.waterfall:
            ai = receiver.audio_in
            self.search_grid = [np.ones((GRID_ROWS, ai.search_grid.shape[1]), np.float32) for _ in range(self.n_channels)]
            d = int(round(ai.waterfall_data["df"] / ai.df))             # the 12 kHz path's downsampling (receiver.WATERFALL_DOWNSAMPLE)
            self.waterfall_data = [dict(ai.waterfall_data, data=g[::d, ::d].T) for g in self.search_grid]

    def _start(self, chunk):
        """The first chunk decides the sample kind and the number of streams, sets the clock and opens the device stream."""
        _, self.kind, self.n_streams, _ = pack(chunk, self.iq, self.sample_rate, self.mod)
        self.src = sources(self.mod, self.src, self.n_streams, self.n_channels)
        if self.t_first is None:
            self.t_first = self._rx.time_source()
        if self.modes is None:
            self.sched = PassScheduler(self.t_first, self._rx.early_decode_hops)
        else:                                    # one scheduler per mode present; `sched` is the FT8 geometry (the grid's rows are mode-blind)
            make = {FT8: lambda: PassScheduler(self.t_first, self._rx.early_decode_hops),
                    FT4: lambda: ft4_scheduler(self.t_first, self._rx.ft4_early_samples)}
            self.scheds = {m: make[m]() for m in self.channels}
            self.sched = self.scheds.get(FT8) or PassScheduler(self.t_first)
        with self._rx._live_lock:
            h = self._rx._live_handle(self.n_channels)
            ib = input_blanker_params(self.input_blanker, self.kind, self.n_streams, self.sample_rate)
            self.f_mixed_hz = HANDLE_CALLS[self.mod][1](h, self.kind, self.sample_rate, self.n_streams, self.src, self.dials,
                                                        2 if self.float_frames else False)
            if ib is not None:
                h.blank_in_stream_open(self.kind, *ib, n_origin=0, max_push=self.sample_rate)
                self._ib = ib
            if self._pan is not None:
                _pan.one_stream(self._pan_opt, self.n_streams)
                n_fft, n_avg, rows = self._pan
                h.pan_stream_open(self.kind, n_fft, n_avg, rows, n_origin=0, max_push=self.sample_rate)
                integer = _kinds.is_integer(self.kind)
                self.panorama = {"data": np.zeros((rows, _pan.bins(self.kind, n_fft)), np.float32),
                                 "stats": np.zeros((rows, 2), np.int64) if integer else None, "r_next": 0,
                                 "f_hz": _pan.freqs(self.kind, self.sample_rate, n_fft), "row_seconds": n_fft * n_avg / float(self.sample_rate),
                                 "n_fft": n_fft, "n_avg": n_avg}
            if self.waterfall:                   # the rows of every hop of the scheduler's cycles, behind whichever stream was opened
                c0 = self.sched.cycle
                self._grid_c0 = (c0, self.sched.cycle_start(c0))
                self.grid_phase = grid_phase(self._grid_c0[1])
                self._grid_q = grid_hops_done(0, self.grid_phase)
                h.ddc_stream_grid_open(self.grid_phase, GRID_ROWS)

    def _push(self, a, real):
        """One chunk of at most a second ([n_streams][n], packed) to the device; real: it counts as source samples.  waterfall: the
        rows the chunk completed are read once and written in place into search_grid"""
        with self._rx._live_lock:
            h = self._rx._live_handle(self.n_channels)
            if self._ib is not None and real:
                self._forward(h, h.blank_in_stream_push(a[0]), _kinds.sample_bytes(self.kind))
            elif self.panorama is not None and real:         # the chunk crosses once, into the panorama's buffer; the front end reads it there
                d_samples, r_done = h.pan_stream_push(a[0])
                self.m_produced = HANDLE_CALLS[self.mod][4](h, d_samples, a.shape[1])
                self._pan_read(h, r_done)
            else:
                self.m_produced = HANDLE_CALLS[self.mod][2](h, a)
            if self.waterfall:
                q_first, q_end = grid_rows_completed(0, self.m_produced, self.grid_phase)
                q_first = max(q_first, self._grid_q)
                if q_end > q_first:
                    rows = h.ddc_stream_grid_read(q_first, q_end - q_first)
                    c0, m_c0 = self._grid_c0
                    for i in range(q_end - q_first):
                        r = grid_place(q_first + i, m_c0, c0)[2]
                        for j, g in enumerate(self.search_grid):
                            g[r, :] = rows[j, i, :g.shape[1]]
                    self._grid_q = q_end
        if real:
            self.n_pushed += a.shape[1]

    def _forward(self, h, released, sample_bytes):
        """What the input blanker released (d_out, n_first, n_out) to the front end's device push, a second at a time; nothing
        released, nothing pushed"""
        d_out, _, n_out = released
        for at in range(0, n_out, self.sample_rate):
            if self.panorama is not None:
                self._pan_read(h, h.pan_stream_push(None, d_ptr=d_out + at * sample_bytes, n=min(self.sample_rate, n_out - at))[1])
            self.m_produced = HANDLE_CALLS[self.mod][4](h, d_out + at * sample_bytes, min(self.sample_rate, n_out - at))

    def _pan_read(self, h, r_done):
        """The rows the last push finished, read once and written in place: row r at r mod rows"""
        p = self.panorama
        n_rows = len(p["data"])
        r0 = max(p["r_next"], r_done - n_rows)
        if r_done > r0:
            rows, stats = h.pan_stream_read(r0, r_done - r0)
            at = np.arange(r0, r_done) % n_rows
            p["data"][at] = rows
            if stats is not None:
                p["stats"][at] = stats
            p["r_next"] = r_done

    def panorama_time(self, r):
        """The time of the first sample of panorama row r on the scheduler's clock: t_first + r n_avg n_fft / sample_rate"""
        if self._pan is None or self.t_first is None:
            return None
        return self.t_first + int(r) * self._pan[0] * self._pan[1] / float(self.sample_rate)

    def input_blanker_stats(self):
        """The input blanker's cumulative int64 [4] (hits, samples with w < 32768, with w = 0, blocks with L_b = 0), or None"""
        if self._ib is None:
            return None
        with self._rx._live_lock:
            return self._rx._live_handle(self.n_channels).blank_in_stream_info()["stats"]

    def grid_cycle(self, odd_even):
        """The newest cycle of parity odd_even whose 375 rows are all in search_grid, or None"""
        if not self.waterfall or self._grid_q is None:
            return None
        c0, m_c0 = self._grid_c0
        c = c0 + (self._grid_q - 1 - grid_row_of(c0, 0, m_c0, c0)) // HOPS_PER_CYCLE - 1
        c -= (c - int(odd_even)) % 2
        return c if c >= c0 else None            # (the cycle before the first one the scheduler decodes is never whole)

    def cycle_spectrum(self, channel, odd_even):
        """The cycle spectrum (complex64 [spec_bins]) of channel `channel`'s frame of grid_cycle(odd_even): the frame whose hops the
        rows of that half of search_grid[channel] are, gathered out of the down-converter's ring (Candidate.decode's fine step)"""
        c = self.grid_cycle(odd_even)
        if c is None:
            raise _lib.Ft8rxError(f"cycle_spectrum: no complete cycle of parity {odd_even} is in the grid of the channels yet")
        if self._spec_cache[0] != c:
            c0, m_c0 = self._grid_c0
            with self._rx._live_lock:
                h = self._rx._live_handle(self.n_channels)
                if self.float_frames:
                    h.ddc_stream_frame_f32(m_c0 + NSAMP * (c - c0), NSAMP)
                    frames = h.download_audio_f32(h.staging_ptr_f32(), self.n_channels)
                else:
                    h.ddc_stream_frame(m_c0 + NSAMP * (c - c0), NSAMP)
                    frames = h.download_audio(h.staging_ptr(), self.n_channels)
            self._spec_cache = (c, frames, {})
        _, frames, specs = self._spec_cache
        if channel not in specs:
            with self._rx._hlock:
                h1 = self._rx._handle(1)
                specs[channel] = (h1.cycle_spectrum_f32 if self.float_frames else h1.cycle_spectrum)(frames[channel])[0]
        return specs[channel]

    def _outputs(self, n):
        """12 kHz outputs that n input samples span, rounded up: ceil(n 12000 / sample_rate), in integers"""
        return -(-int(n) * 12000 // self.sample_rate)

    def _note(self, m_avail):
        due = self.sched.due(m_avail) if self.scheds is None else merge_due({m: s.due(m_avail) for m, s in self.scheds.items()})
        if due:
            with self._lock:
                self._ready += due

    def push(self, chunk):
        """The next samples of the source, any length (a longer chunk is handed on a second at a time)"""
        if self.sched is None:
            self._start(chunk)
        a, _, n_streams, n = pack(chunk, self.iq, self.sample_rate, self.mod, self.kind)
        if n_streams != self.n_streams:
            raise _lib.Ft8rxError(f"push: {n_streams} streams, the source began with {self.n_streams}")
        for at in range(0, n, self.sample_rate):
            self._push(a[:, at:at + self.sample_rate], True)
            self._note(self.m_produced)

    def flush(self):
        """End of a finite source: zeros until the outputs of the last real sample exist; the passes those outputs complete"""
        if self.sched is None:
            return
        m_real = self._outputs(self.n_pushed)
        if self._ib is not None:                 # the blanker's stream ends here: what it still holds goes on, the zeros go past it
            with self._rx._live_lock:
                h = self._rx._live_handle(self.n_channels)
                if not self._ib_done:
                    self._ib_done = True
                    self._forward(h, h.blank_in_stream_push(None, finish=True), _kinds.sample_bytes(self.kind))
        # a tile's worth of rest samples per stream, rounded up (1008 D at a multiple of 12 kHz); uint8 has no zero: 128 is half a step,
        # 128 counts of the int16 scale, above it
        dtype = _kinds.DTYPE[self.kind]
        zeros = np.full((self.n_streams,) + _kinds.shape(self.kind, -(-TILE * self.sample_rate // 12000)), 128 if dtype == np.uint8 else 0, dtype)
        while self.m_produced < m_real:
            self._push(zeros, False)
        self._note(m_real)

    def open(self, source):
        """Feed push() from an iterator of chunks on a daemon thread.  Pacing is the iterator's business (a live source blocks until
        its next chunk exists; a test advances its virtual clock inside the generator)."""
        def feed():
            try:
                for chunk in source:
                    if self._rx._stop.is_set():
                        break
                    self.push(chunk)
                else:
                    self.flush()
                    self.source_exhausted = True
            except Exception as e:          # noqa: BLE001 -- surfaced by Receiver.poll()/stop() instead of dying silently on a daemon thread
                self._rx.thread_error = e
            finally:
                self._feeder = None
        self.source_exhausted = False
        t = self._feeder = _threading.Thread(target=feed, name="ft8rx-wide-in", daemon=True)
        t.start()
        return self

    def close(self, timeout=5.0):
        """Wait for the feeder thread (it ends at its next chunk once the receiver's stop flag is set)."""
        t = self._feeder
        if t is not None and t is not _threading.current_thread():
            t.join(timeout)
            if not t.is_alive():
                self._feeder = None
