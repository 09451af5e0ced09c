"""Measure the input-rate noise blanker (ft8rx_blank_in_stream_push) on the GPU and write the measured section
of profiles/blank_in_notes.md:
  * one push of 40 ms and of 1 s at 2.4 MS/s IQ uint8 and at 64.8 MS/s real int16, from device memory, clean noise and with 100
    impulses per second of 100 sigma: host clock around the queued push and the handle's synchronise, warm-up first, median of the
    timed repeats;
  * beside it, in the same run, ft8rx_ddc_wide_stream_push (one channel) of the same chunk from device memory;
  * the decode counts of the 240 kHz recipe of tests/blank_in_cases.py on the GPU (decode_stream: clean, with impulses, noise_blanker
    only, input_blanker only).
For the kernels' own times run it under `rocprofv3 --kernel-trace --stats -- python tools/blank_in_measure.py --no-counts`, in a run
of its own.
Usage: python tools/blank_in_measure.py [--repeats 10] [--no-counts] [--out profiles/blank_in_notes.md]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pyft8_amd import _lib  # noqa: E402
from pyft8_amd import blank_in as bi  # noqa: E402

MARK = "## Measured (tools/blank_in_measure.py)"
CASES = (("2.4 MS/s IQ uint8", bi.WIDE_IQ_U8, 2400000), ("64.8 MS/s real int16", bi.WIDE_REAL_I16, 64800000))


def chunk(kind, rate, n, impulses, seed):
    rng = np.random.default_rng(seed)
    if kind == bi.WIDE_IQ_U8:
        x = np.clip(np.rint(127.5 + 10.0 * rng.standard_normal((n, 2), dtype=np.float32)), 0, 255).astype(np.uint8)
    else:
        x = np.rint(1000.0 * rng.standard_normal(n, dtype=np.float32)).astype(np.int16)
    return bi.add_impulses(x, kind, rng, 100.0, rate, 100.0) if impulses else x


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
        block = bi.block_for_rate(rate)
        for seconds in (0.04, 1.0):
            n = int(round(seconds * rate))
            for impulses in (False, True):
                d = torch.from_numpy(chunk(kind, rate, n, impulses, 5)).to(dev)
                torch.cuda.synchronize()
                h.blank_in_stream_open(kind, block, max_push=n)
                s0 = h.blank_in_stream_info()["stats"]
                t_bi = timed(lambda: h.blank_in_stream_push(None, d_ptr=d.data_ptr(), n=n), h.sync, repeats, warmup)
                hits = (h.blank_in_stream_info()["stats"] - s0)[0] / float(repeats + warmup)
                h.blank_in_stream_close()
                h.ddc_wide_stream_open(kind, rate, [0.1 * rate])
                t_dw = timed(lambda: h.ddc_wide_stream_push(None, d_ptr=d.data_ptr(), n=n), h.sync, repeats, warmup)
                h.ddc_wide_stream_close()
                rows.append({"input": name, "push_s": seconds, "samples": n, "block": block, "impulses": impulses, "hits_per_push": hits,
                             "blank_in_us": [1e3 * v for v in t_bi], "ddc_wide_us": [1e3 * v for v in t_dw],
                             "bytes_per_s_3_passes": 3.0 * d.numel() * d.element_size() / (t_bi[0] * 1e-3)})
                del d
    h.close()
    return rows


def recipe_counts():
    import blank_in_cases as cases
    from pyft8_amd.receiver import Receiver
    names = ("clean", "impulses", "impulses, noise_blanker=True", "impulses, input_blanker=True")
    res = {n: {"true": 0, "false": 0} for n in names}
    for clean, noisy, f_off, _, truth in cases.benefit_recipe():
        for n, x, kw in zip(names, (clean, noisy, noisy, noisy), ({}, {}, {"noise_blanker": True}, {"input_blanker": True})):
            rx = Receiver("", None, max_frames=1, **kw)
            try:
                texts = [" ".join(d["msg_tuple"]) for d in rx.decode_stream(x, cases.BENEFIT_RATE, iq=True, dial_offsets_hz=[f_off])[0]]
            finally:
                rx.close()
            res[n]["true"] += sum(t in truth for t in texts)
            res[n]["false"] += sum(t not in truth for t in texts)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-counts", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blank_in_notes.md"))
    a = ap.parse_args()
    res = {"repeats": a.repeats, "warmup": a.warmup, "pushes": measure_pushes(a.repeats, a.warmup)}
    if not a.no_counts:
        res["recipe"] = recipe_counts()
    print(json.dumps(res))
    lines = [MARK, "",
             f"One push from device memory, host clock around the queued call and `ft8rx_sync`, {a.warmup} warm-up pushes, median (min .. max) of "
             f"{a.repeats}; `block` = the default of the rate, k / guard / taper the defaults; beside it `ft8rx_ddc_wide_stream_push` (one channel) of "
             "the same chunk in the same run.  GB/s counts three passes over the chunk.", "",
             "| input | push | impulses | hits / push | blank_in us | ddc_wide us | GB/s (3 passes) |", "|---|---|---|---|---|---|---|"]
    for r in res["pushes"]:
        b, w = r["blank_in_us"], r["ddc_wide_us"]
        lines.append(f"| {r['input']} | {r['push_s'] * 1e3:.0f} ms | {'100 / s' if r['impulses'] else 'none'} | {r['hits_per_push']:.0f} | "
                     f"{b[0]:.0f} ({b[1]:.0f} .. {b[2]:.0f}) | {w[0]:.0f} ({w[1]:.0f} .. {w[2]:.0f}) | {r['bytes_per_s_3_passes'] / 1e9:.0f} |")
    if "recipe" in res:
        lines += ["", "Decode counts of the 240 kHz recipe on the GPU (`Receiver.decode_stream`, tests/blank_in_cases.py: benefit_recipe):", "",
                  "| input | true | false |", "|---|---|---|"]
        lines += [f"| {n} | {c['true']} | {c['false']} |" for n, c in res["recipe"].items()]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    head = open(a.out).read().split(MARK)[0] if os.path.exists(a.out) else ""
    with open(a.out, "w") as f:
        f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
