"""Measure the noise blanker (ft8rx_blank) on the GPU and write profiles/blanker_notes.md:
  * the call on 256 resident frames, host clock around the queued call and the handle's synchronise, warm-up first, median of the timed
    repeats -- on clean frames (no hit: the gate returns without touching the audio) and on the impulse recipe (100 impulses per second);
    the input is restored from a pristine device copy before every repeat, outside the timed window (the call works in place);
  * the config-1 step (bench.py --gpus 1) of the parent commit -- a built checkout of it given with --parent-tree, its own bench.py on
    its own library -- and of this build, option off, alternating, each in a process of its own;
  * the decode counts of the recipe: true / false messages of the clean frames, with impulses, and with noise_blanker=True.
For the kernels' own times run it under `rocprofv3 --kernel-trace --stats -- python tools/blanker_measure.py --no-bench --no-counts`.
Usage: python tools/blanker_measure.py [--frames 256] [--repeats 30] [--parent-tree DIR] [--out profiles/blanker_notes.md]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyft8_amd import _lib, blanker, synth  # noqa: E402
from pyft8_amd.receiver import Receiver  # noqa: E402

HBM_PEAK = 8.0e12                      # bytes per second, the figure DESIGN.md section 6 uses for every kernel
FRAME_BYTES = 2 * _lib.NSAMP


def time_call(h, d, pristine, B, q8, guard, taper, repeats, warmup, want_stats):
    ms = []
    for i in range(warmup + repeats):
        d.copy_(pristine)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.blank(d.data_ptr(), B, q8, guard, taper, want_stats=want_stats)
        h.sync()
        if i >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    return ms


def measure_call(B, repeats, warmup):
    dev = torch.device("cuda", 0)
    h = _lib.Handle(device=0, max_frames=B)
    clean = torch.empty((B, _lib.NSAMP), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    h.synth_frames(clean.data_ptr(), 0, B, n_signals=30, snr_range=(-16.0, 0.0))
    h.sync()
    host = clean.cpu().numpy()
    rng = np.random.default_rng(17)
    noisy = torch.from_numpy(np.stack([blanker.add_impulses(f, rng, 100.0, 30.0) for f in host])).to(dev)
    d = torch.empty_like(clean)
    q8, guard, taper = blanker.check()
    out = {}
    for name, src in (("clean", clean), ("impulses", noisy)):
        d.copy_(src)
        torch.cuda.synchronize()
        stats = h.blank(d.data_ptr(), B, q8, guard, taper)
        queued = time_call(h, d, src, B, q8, guard, taper, repeats, warmup, False)
        with_stats = time_call(h, d, src, B, q8, guard, taper, repeats, warmup, True)
        med = statistics.median(queued)
        out[name] = {"hits_per_frame": float(stats[:, 0].mean()), "gated_samples_per_frame": float(stats[:, 1].mean()),
                     "us_median": 1e3 * med, "us_min": 1e3 * min(queued), "us_max": 1e3 * max(queued),
                     "us_median_with_stats": 1e3 * statistics.median(with_stats),
                     "fraction_of_hbm_peak_3_passes": 3.0 * FRAME_BYTES * B / (med * 1e-3) / HBM_PEAK}
    h.close()
    return out


def bench_step(tree, steps, warmup):
    p = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       cwd=tree, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"bench.py failed ({p.returncode}): {p.stderr[-2000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    j = json.loads(line)
    return {"ms_per_step": j["ms_per_step"], "frames_per_s": j["value"]}


def recipe_counts():
    rng = np.random.default_rng(17)
    clean, noisy, truth = [], [], []
    for i in (900, 901, 902):
        x, t = synth.make_frame(i, n_signals=30, snr_range=(-16, 0), return_truth=True)
        clean.append(x)
        noisy.append(blanker.add_impulses(x, rng, 100.0, 30.0))
        truth.append({m["msg"] for m in t})
    clean, noisy = np.stack(clean), np.stack(noisy)
    res = {}
    for name, frames, nb in (("clean", clean, None), ("impulses", noisy, None), ("impulses, noise_blanker=True", noisy, True),
                             ("clean, noise_blanker=True", clean, True)):
        rx = Receiver("", None, max_frames=3, noise_blanker=nb)
        try:
            out = rx.decode_frames(frames)
            hits = None if rx.blanker_stats is None else [int(v) for v in rx.blanker_stats[:, 0]]
        finally:
            rx.close()
        texts = [[" ".join(d["msg_tuple"]) for d in o] for o in out]
        res[name] = {"true": sum(x in t for o, t in zip(texts, truth) for x in o), "false": sum(x not in t for o, t in zip(texts, truth) for x in o),
                     "hits": hits}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (config-1 step without the blanker's code)")
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-rounds", type=int, default=2, help="bench.py runs per build, alternating")
    ap.add_argument("--this-first", action="store_true", help="start the alternation with this build instead of the parent's")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--no-counts", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blanker_notes.md"))
    a = ap.parse_args()
    res = {"frames": a.frames, "repeats": a.repeats, "warmup": a.warmup}
    if not a.no_bench:
        builds = [("this build", ROOT)]
        if a.parent_tree:
            builds.insert(1 if a.this_first else 0, ("parent build", os.path.abspath(a.parent_tree)))
        res["config1"] = {n: [] for n, _ in builds}
        for _ in range(a.bench_rounds):
            for n, tree in builds:
                res["config1"][n].append(bench_step(tree, a.bench_steps, 10))
    res["call"] = measure_call(a.frames, a.repeats, a.warmup)
    if not a.no_counts:
        res["recipe"] = recipe_counts()
    print(json.dumps(res))
    lines = ["## Measured (tools/blanker_measure.py)", "",
             f"`ft8rx_blank` on {a.frames} resident frames, k = 8, guard 6, taper 6; host clock around the queued call and `ft8rx_sync`, "
             f"{a.warmup} warm-up calls, median of {a.repeats}; the fraction of HBM peak counts 3 x 360 KB per frame (two reads, one write) "
             "against 8 TB/s.", "",
             "| frames | hits / frame | gated samples / frame | median us | min .. max us | median us with stats | fraction of HBM peak |",
             "|---|---|---|---|---|---|---|"]
    for n, c in res["call"].items():
        lines.append(f"| {n} | {c['hits_per_frame']:.0f} | {c['gated_samples_per_frame']:.0f} | {c['us_median']:.1f} | {c['us_min']:.1f} .. {c['us_max']:.1f} | "
                     f"{c['us_median_with_stats']:.1f} | {c['fraction_of_hbm_peak_3_passes']:.3f} |")
    if "config1" in res:
        lines += ["", f"Config-1 step (`bench.py --gpus 1 --steps {a.bench_steps} --warmup 10`, option off), runs alternating, a process each:", "",
                  "| build | ms per step | frames/s |", "|---|---|---|"]
        for n, runs in res["config1"].items():
            ms = ", ".join("%.3f" % r["ms_per_step"] for r in runs)
            fps = ", ".join("%.0f" % r["frames_per_s"] for r in runs)
            lines.append(f"| {n} | {ms} | {fps} |")
    if "recipe" in res:
        lines += ["", "Decode counts of the recipe on the GPU (`Receiver.decode_frames`, frames 900 .. 902, 30 signals at -16 .. 0 dB, 100 impulses "
                  "per second of 30 sigma x U[0.5, 1.5]):", "", "| frames | true | false | hits per frame |", "|---|---|---|---|"]
        for n, c in res["recipe"].items():
            lines.append(f"| {n} | {c['true']} | {c['false']} | {c['hits'] if c['hits'] is not None else '-'} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    head = ""
    if os.path.exists(a.out):                       # keep the hand-written part above the measured section
        head = open(a.out).read().split("## Measured (tools/blanker_measure.py)")[0]
    with open(a.out, "w") as f:
        f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
