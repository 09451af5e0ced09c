"""Cost of the opt-in message types (config msg_types) on the GPU:

  1. extra messages per frame on noise-only frames at default kwargs (and at a lowered sync threshold), msg_types="all" vs the
     default -- false decodes by construction (there is no signal), split by message type and decode method;
  2. Receiver.decode_frames wall time on the config-1 workload (BASELINE: 256 frames of 50 signals at -10 .. +10 dB, which carries no
     message of the new types), default vs "all", alternating runs; with the new-type (false) decodes and default messages lost.

    python tools/msg_types_measure.py [--noise-frames 2048] [--frames 256] [--reps 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time
from collections import Counter

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyft8_amd import _lib, synth  # noqa: E402
from pyft8_amd.receiver import Receiver  # noqa: E402


def kind(m):
    """'<msg_type> <method>' of a message dict (method: the last field of decode_notes)."""
    return m["msg_type"] + " " + m["decode_notes"].split("_")[-1].split(" ")[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--noise-frames", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--noise-sync-min", type=float, default=20.0, help="second noise run: sync_score_min (default kwargs: 85)")
    a = ap.parse_args()
    res = {"noise_frames": a.noise_frames}
    # 1. noise only: at default kwargs, and with the sync threshold lowered so that candidates reach the decoder at all
    for smin in (85, a.noise_sync_min):
        rx0 = Receiver("", None, max_frames=a.frames, sync_score_min=smin)
        rx1 = Receiver("", None, max_frames=a.frames, sync_score_min=smin, msg_types="all")
        rng = np.random.default_rng(20261015)
        n0 = n1 = 0
        kinds = Counter()
        for lo in range(0, a.noise_frames, a.frames):
            B = min(a.frames, a.noise_frames - lo)
            audio = np.clip(np.rint(rng.standard_normal((B, synth.NFRAME)) * 1000.0), -32768, 32767).astype(np.int16)
            d0, d1 = rx0.decode_frames(audio), rx1.decode_frames(audio)
            n0 += sum(map(len, d0))
            n1 += sum(map(len, d1))
            for f in d1:
                for m in f:
                    kinds[kind(m)] += 1
        res[f"noise_sync_score_min_{smin}"] = dict(msgs_per_frame_default=n0 / a.noise_frames, msgs_per_frame_all=n1 / a.noise_frames,
                                                   extra_per_frame=(n1 - n0) / a.noise_frames, all_mode_by_type_and_method=dict(sorted(kinds.items())))
        rx0.close()
        rx1.close()
    rx0 = Receiver("", None, max_frames=a.frames)
    rx1 = Receiver("", None, max_frames=a.frames, msg_types="all")
    # 2. decode_frames timing on the config-1 workload
    h = _lib.Handle(max_frames=a.frames)
    h.synth_frames(h.staging_ptr(), 0, a.frames, n_signals=50, snr_range=(-10.0, 10.0))
    audio = h.download_audio(h.staging_ptr(), a.frames)
    h.close()
    for rx in (rx0, rx1):                      # warm-up
        rx.decode_frames(audio)
    t = {0: [], 1: []}
    for _ in range(a.reps):
        for k, rx in ((0, rx0), (1, rx1)):
            t0 = time.perf_counter()
            d = rx.decode_frames(audio)
            t[k].append(time.perf_counter() - t0)
            if k == 0:
                ref = d
            else:
                got = d
    # the workload carries no message of the new types: every one "all" mode emits is a false decode; a default message missing
    # from "all" mode is a candidate whose ladder a CRC-valid word of a new type stopped before it reached the true word
    lost = sum(len({m["msg_tuple"] for m in x} - {m["msg_tuple"] for m in y}) for x, y in zip(ref, got))
    new_kinds = Counter(kind(m) for f in got for m in f if m["msg_type"] not in ("1", "2", "4"))
    med = {k: float(np.median(v)) for k, v in t.items()}
    res.update(config1_msgs_per_frame_default=sum(map(len, ref)) / a.frames, config1_msgs_per_frame_all=sum(map(len, got)) / a.frames,
               config1_new_type_per_frame=sum(new_kinds.values()) / a.frames, config1_new_type_by_type_and_method=dict(sorted(new_kinds.items())),
               config1_default_messages_lost_per_frame=lost / a.frames)
    res.update(decode_frames_ms_default=1e3 * med[0], decode_frames_ms_all=1e3 * med[1],
               frames_per_s_default=a.frames / med[0], frames_per_s_all=a.frames / med[1],
               spread_ms_default=[1e3 * min(t[0]), 1e3 * max(t[0])], spread_ms_all=[1e3 * min(t[1]), 1e3 * max(t[1])],
               frames=a.frames, reps=a.reps)
    rx0.close()
    rx1.close()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
