"""Measure the panorama (ft8rx_pan_stream_push) on the GPU and write the measured section of
profiles/pan_notes.md:
  * one push of 40 ms and of 1 s at 2.4 MS/s IQ uint8 and at 64.8 MS/s real int16, from device memory, at the default n_fft and the
    rate's default n_avg: host clock around the queued push and the handle's synchronise, warm-up first, median of the timed repeats;
  * beside it, in the same run, ft8rx_ddc_wide_stream_push (one channel) of the same chunk from device memory;
  * achieved bytes per second by algorithmic bytes: the input once, plus the window powers written by k_pan_power and read back by
    k_pan_rows (the scratch the plain window order costs).
For the kernels' own times run it under `rocprofv3 --kernel-trace --stats -- python tools/pan_measure.py`, in a run of its own.
Usage: python tools/pan_measure.py [--repeats 10] [--out profiles/pan_notes.md]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyft8_amd import _lib  # noqa: E402
from pyft8_amd import kinds as K  # noqa: E402
from pyft8_amd import pan  # noqa: E402

MARK = "## Measured (tools/pan_measure.py)"
CASES = (("2.4 MS/s IQ uint8", K.WIDE_IQ_U8, 2400000), ("64.8 MS/s real int16", K.WIDE_REAL_I16, 64800000))


def chunk(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == K.WIDE_IQ_U8:
        return np.clip(np.rint(127.5 + 10.0 * rng.standard_normal((n, 2), dtype=np.float32)), 0, 255).astype(np.uint8)
    return np.rint(1000.0 * rng.standard_normal(n, dtype=np.float32)).astype(np.int16)


def timed(push, sync, repeats, warmup):
    ms = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        push()
        sync()
        if i >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms), min(ms), max(ms)


def measure_pushes(repeats, warmup):
    dev = torch.device("cuda", 0)
    h = _lib.Handle(device=0, max_frames=1)
    rows = []
    for name, kind, rate in CASES:
        n_fft, n_avg, n_rows = pan.params(True, rate)
        for seconds in (0.04, 1.0):
            n = int(round(seconds * rate))
            d = torch.from_numpy(chunk(kind, n, 5)).to(dev)
            torch.cuda.synchronize()
            h.pan_stream_open(kind, n_fft, n_avg, n_rows, max_push=n)
            t_pan = timed(lambda: h.pan_stream_push(None, d_ptr=d.data_ptr(), n=n), h.sync, repeats, warmup)
            h.pan_stream_close()
            h.ddc_wide_stream_open(kind, rate, [0.1 * rate])
            t_dw = timed(lambda: h.ddc_wide_stream_push(None, d_ptr=d.data_ptr(), n=n), h.sync, repeats, warmup)
            h.ddc_wide_stream_close()
            in_bytes = d.numel() * d.element_size()
            pw_bytes = 2 * 4 * (n // n_fft) * pan.bins(kind, n_fft)
            rows.append({"input": name, "push_s": seconds, "samples": n, "n_fft": n_fft, "n_avg": n_avg, "pan_us": [1e3 * v for v in t_pan],
                         "ddc_wide_us": [1e3 * v for v in t_dw], "input_bytes": in_bytes, "power_bytes": pw_bytes,
                         "bytes_per_s": (in_bytes + pw_bytes) / (t_pan[0] * 1e-3)})
            del d
    h.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pan_notes.md"))
    a = ap.parse_args()
    res = {"repeats": a.repeats, "warmup": a.warmup, "pushes": measure_pushes(a.repeats, a.warmup)}
    print(json.dumps(res))
    lines = [MARK, "",
             f"One push from device memory (one device-to-device copy of the chunk included), host clock around the queued call and `ft8rx_sync`, "
             f"{a.warmup} warm-up pushes, median (min .. max) of {a.repeats}; n_fft 2048, n_avg the rate's default; beside it "
             "`ft8rx_ddc_wide_stream_push` (one channel) of the same chunk in the same run.  GB/s counts the algorithmic bytes: the input once plus "
             "the window powers written and read back once.", "",
             "| input | push | n_avg | panorama us | ddc_wide us | input MB | powers MB (w + r) | GB/s |", "|---|---|---|---|---|---|---|---|"]
    for r in res["pushes"]:
        b, w = r["pan_us"], r["ddc_wide_us"]
        lines.append(f"| {r['input']} | {r['push_s'] * 1e3:.0f} ms | {r['n_avg']} | {b[0]:.0f} ({b[1]:.0f} .. {b[2]:.0f}) | {w[0]:.0f} ({w[1]:.0f} .. {w[2]:.0f}) | "
                     f"{r['input_bytes'] / 1e6:.1f} | {r['power_bytes'] / 1e6:.1f} | {r['bytes_per_s'] / 1e9:.1f} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    head = open(a.out).read().split(MARK)[0] if os.path.exists(a.out) else ""
    with open(a.out, "w") as f:
        f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
