"""Time live FT4 on the GPU: K FT4 channels out of ONE 192 kHz IQ int16 stream, every channel carrying six
signals per 7.5-s slot (ft4.make_frame), pushed from host memory in 40-ms chunks as a live source does, with a poll() after every push
that made a pass due.  Prints one JSON line per K, host-to-host milliseconds:
  early_ms / complete_ms   from the return of the push that made the pass due (its outputs exist once the push's kernel has run; the
                           wait for it is inside) to the last on_message of that pass: gather, decode of the K frames as one batch,
                           fetch, host message layer, delivery.  The first slot is left out (the handle's first FT4 call allocates).
  messages                 delivered per slot and channel, early and in all
  gather_ms                ft8rx_ddc_stream_frames alone for the K channels at either frame length, and ft8rx_ddc_stream_frame beside it
                           (every timed call ends in ft8rx_sync)
Usage: python tools/ft4_live_measure.py [K ...] [--slots N] [--passes P]     (default K = 1 16, 4 slots, one pass)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401 -- imported before libft8rx.so loads (pyft8_amd/_lib.py: lib)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyft8_amd import _lib, ft4  # noqa: E402
from pyft8_amd.receiver import Receiver  # noqa: E402

RATE, SLOT = 192000, ft4.NFRAME


def stats(ms):
    ms = sorted(ms)
    return {"min": round(ms[0], 3), "median": round(ms[len(ms) // 2], 3), "max": round(ms[-1], 3), "n": len(ms)}


def stream(K, n_slots, dials):
    """IQ int16 [n_slots 90000 x 16, 2]: channel j's slots make_frame(1000 + n_slots j + c) joined, a USB channel at dials[j]"""
    n_audio = n_slots * SLOT
    spec = np.zeros(n_audio * RATE // 12000, np.complex128)
    for j in range(K):
        audio = np.concatenate([ft4.make_frame(1000 + n_slots * j + c) for c in range(n_slots)])
        a = np.fft.rfft(audio.astype(np.float64))[:n_audio // 2].copy()
        a[1:] *= 2.0
        spec[(int(round(dials[j] * n_audio / 12000.0)) + np.arange(len(a))) % len(spec)] += a
    x = np.fft.ifft(spec) * len(spec) / n_audio
    peak = max(np.abs(x.real).max(), np.abs(x.imag).max())
    scale = min(1.0, 30000.0 / peak)                                                    # K channels of unit noise add up: keep int16 headroom
    return np.stack([np.rint(x.real * scale), np.rint(x.imag * scale)], axis=1).astype(np.int16), scale


def measure(K, n_slots, passes):
    dials = [-90000.0 + 11000.0 * j for j in range(K)] if K > 1 else [1000.0]
    x, scale = stream(K, n_slots, dials)
    t_first, stamps = 7.5 * 1000, []
    rx = Receiver("", lambda d: stamps.append((time.perf_counter(), d)), sample_rate=RATE, iq=True, dial_offsets_hz=dials, modes="FT4",
                  t_first=t_first, time_source=lambda: t_first, **({"ft4_passes": passes} if passes > 1 else {}))
    out = {"K": K, "rate_hz": RATE, "slots": n_slots, "ft4_passes": passes, "signals_per_slot": 6, "scale": round(scale, 4)}
    lat = {True: [], False: []}
    counts = []
    chunk = RATE // 25
    try:
        for at in range(0, len(x), chunk):
            rx.wide_in.push(x[at:at + chunk])
            while rx.wide_in._ready:
                c, n_have = rx.wide_in._ready[0][0], rx.wide_in._ready[0][3]
                t0, n0 = time.perf_counter(), len(stamps)
                rx.poll()
                t_last = stamps[-1][0] if len(stamps) > n0 else time.perf_counter()
                if c > 1000:                                                            # the first slot warms up
                    lat[n_have < SLOT].append(1e3 * (t_last - t0))
                    counts.append((n_have < SLOT, len(stamps) - n0))
        rx.wide_in.flush()
        while rx.wide_in._ready:
            t0, n0, n_have = time.perf_counter(), len(stamps), rx.wide_in._ready[0][3]
            rx.poll()
            lat[n_have < SLOT].append(1e3 * ((stamps[-1][0] if len(stamps) > n0 else time.perf_counter()) - t0))
            counts.append((n_have < SLOT, len(stamps) - n0))
        out["early_ms"], out["complete_ms"] = stats(lat[True]), stats(lat[False])
        n_timed = max(1, len(lat[False]))
        out["messages"] = {"early_per_slot_and_channel": round(sum(n for e, n in counts if e) / n_timed / K, 2),
                           "all_per_slot_and_channel": round(sum(n for _, n in counts) / n_timed / K, 2)}
        h = rx._live
        m = h.ddc_stream_info()["m_produced"]

        def timed(fn):
            t0 = time.perf_counter()
            fn()
            h.sync()
            return 1e3 * (time.perf_counter() - t0)
        ch = list(range(K))
        g = {}
        for name, fn in (("frames_90000", lambda: h.ddc_stream_frames(m - SLOT, SLOT, SLOT, ch)),
                         ("frames_180000", lambda: h.ddc_stream_frames(m - _lib.NSAMP, _lib.NSAMP, _lib.NSAMP, ch)),
                         ("frame_180000", lambda: h.ddc_stream_frame(m - _lib.NSAMP, _lib.NSAMP))):
            timed(fn)
            g[name] = stats([timed(fn) for _ in range(20)])
        out["gather_ms"] = g
    finally:
        rx.stop()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("K", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--passes", type=int, default=1)
    a = ap.parse_args()
    for K in a.K:
        if not 1 <= K <= 16:
            raise SystemExit("K: 1 .. 16 channels fit the 192 kHz stream at 11 kHz spacing")
        print(json.dumps(measure(K, a.slots, a.passes)), flush=True)


if __name__ == "__main__":
    main()
