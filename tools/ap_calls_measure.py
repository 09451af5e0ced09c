"""Cost and yield of the opt-in a-priori calls (ft8rx_set_ap_calls, ipass 7) on the GPU:

  1. noise: ipass-7 decodes on device-synthesised noise-only frames with both calls set and the gate wide open (ap_max_hd = 174),
     as a histogram of their distances per method -- the false-decode rate of every threshold, the basis of FT8RX_AP_MAX_HD_DEFAULT;
  2. the config-1 workload (BASELINE: 50 signals at -10 .. +10 dB) with random calls that appear in no transmitted message: false
     ipass-7 decodes per frame, open gate and default gate;
  3. decode rate against SNR per pattern, default vs calls set (frames of synth.frame_from_words carrying one word per pattern);
  3b. the same frames with the gate wide open: distances of the ipass-7 decodes that are the transmitted word (true) and that are not
     (false) -- what a given ap_max_hd costs in sensitivity;
  4. Receiver.decode_frames wall time on 256 config-1 frames, calls unset vs set, alternating runs.

    python tools/ap_calls_measure.py [--noise-frames 2048] [--frames 256] [--reps 10] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time
from collections import Counter

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyft8_amd import _lib, synth  # noqa: E402
from pyft8_amd import messages as M  # noqa: E402
from pyft8_amd.receiver import Receiver  # noqa: E402

MY, DX = "K1ABC", "W9XYZ"
PATTERN_WORDS = {5: (MY, "N0CALL", "-10"), 6: (MY, DX, "R-12"), 7: ("CQ", DX, "FN42"), 8: (MY, DX, "RRR"), 9: (MY, DX, "73"),
                 10: (MY, DX, "RR73")}
METH = {_lib.M_LDPC_B: "BP", _lib.M_OSD: "OSD", _lib.M_AP_CODEWORD: "CODEWORD"}


def device_batches(h, start, n, B, n_signals, **kw):
    d = torch.empty((B, synth.NFRAME), dtype=torch.int16, device="cuda")
    for k in range(0, n, B):
        truth = h.synth_frames(d.data_ptr(), start + k, B, n_signals=n_signals, **kw)
        torch.cuda.synchronize()
        h.enqueue(d.data_ptr(), B)
        yield h.fetch(B), truth


def ipass7(rec, cnt):
    for f in range(len(cnt)):
        for r in rec[f, :cnt[f]]:
            if r["status"] == _lib.ST_DECODED and r["ipass"] == 7:
                yield f, r


def noise(n_frames, B=256):
    h = _lib.Handle(max_frames=B)
    h.set_ap_calls(MY, DX)
    h.set_ap_max_hd(174)
    hist = Counter()
    try:
        for (rec, cnt, _, _), _ in device_batches(h, 20_000_000, n_frames, B, 0):
            for _, r in ipass7(rec, cnt):
                hist[(METH[int(r["method"])], int(r["ap"]), int(r["osd_hd"]))] += 1
    finally:
        h.close()
    rows = sorted(hist.items(), key=lambda kv: kv[0][2])
    return {"frames": n_frames, "calls": [MY, DX], "decodes_open_gate": sum(hist.values()),
            "min_hd": rows[0][0][2] if rows else None,
            "by_method_ap_hd": [[m, ap, hd, n] for (m, ap, hd), n in rows],
            "false_per_frame_at_default_gate": sum(n for (m, ap, hd), n in rows if hd <= _lib.AP_MAX_HD_DEFAULT) / n_frames}


def workload_false(n_frames, B=256):
    rng = np.random.default_rng(99)
    out = {}
    h = _lib.Handle(max_frames=B)
    d = torch.empty((B, synth.NFRAME), dtype=torch.int16, device="cuda")
    try:
        for gate in (174, _lib.AP_MAX_HD_DEFAULT):
            n7, hds, frames = 0, [], 0
            for k in range(0, n_frames, B):
                truth = h.synth_frames(d.data_ptr(), k, B, n_signals=50, snr_range=(-10.0, 10.0))
                torch.cuda.synchronize()
                sent = " ".join(t["msg"] for fr in truth for t in fr)
                while True:
                    my, dx = synth.random_call(rng), synth.random_call(rng)
                    if my not in sent and dx not in sent:
                        break
                h.set_ap_calls(my, dx)
                h.set_ap_max_hd(gate)
                h.enqueue(d.data_ptr(), B)
                rec, cnt, _, _ = h.fetch(B)
                for _, r in ipass7(rec, cnt):
                    n7 += 1
                    hds.append(int(r["osd_hd"]))
                frames += B
            out[f"gate_{gate}"] = {"frames": frames, "ipass7_per_frame": n7 / frames, "min_hd": min(hds) if hds else None,
                                   "hd_histogram": {str(k): v for k, v in sorted(Counter(hds).items())}}
    finally:
        h.close()
    return out


def rate_vs_snr(snrs, n_frames):
    words = [synth.pack77(*PATTERN_WORDS[p]) for p in range(5, 11)]
    texts = [" ".join(M.unpack(w, M.CallHashes())) for w in words]
    res = []
    for snr in snrs:
        audio = np.stack([synth.frame_from_words(40000 + i, words, snr_range=(snr, snr)) for i in range(n_frames)])
        row = {"snr": snr, "frames": n_frames}
        for mode, kw in (("default", {}), ("ap", dict(my_call=MY, dx_call=DX))):
            rx = Receiver("", None, max_frames=n_frames, **kw)
            try:
                d = rx.decode_frames(audio)
            finally:
                rx.close()
            hits = [0] * 6
            for f in d:
                for k, t in enumerate(texts):
                    f0 = 300.0 + 2400.0 * (k + 0.5) / 6
                    hits[k] += any(" ".join(m["msg_tuple"]) == t and abs(m["fHz"] - f0) < 15 for m in f)
            row[mode] = dict(zip([M.AP_CALL_NAMES[p - 5] + " (" + " ".join(PATTERN_WORDS[p]) + ")" for p in range(5, 11)], hits))
        res.append(row)
        print(json.dumps(row), flush=True)
    return res


def true_distances(snrs, n_frames):
    """ipass-7 decodes of the rate_vs_snr frames with ap_max_hd = 174: distance histograms of true and false words per method, and
    how many true ones a gate keeps."""
    words = [synth.pack77(*PATTERN_WORDS[p]) for p in range(5, 11)]
    sent = set(words)
    true, false = Counter(), Counter()
    h = _lib.Handle(max_frames=n_frames)
    try:
        h.set_ap_calls(MY, DX)
        h.set_ap_max_hd(174)
        for snr in snrs:
            audio = np.stack([synth.frame_from_words(40000 + i, words, snr_range=(snr, snr)) for i in range(n_frames)])
            rec, cnt, _, _ = h.decode_batch(audio)
            for _, r in ipass7(rec, cnt):
                w = (int(r["msg_hi"]) << 64) | int(r["msg_lo"])
                (true if w in sent else false)[(METH[int(r["method"])], int(r["osd_hd"]))] += 1
    finally:
        h.close()
    hist = lambda c: {m: {str(hd): n for (mm, hd), n in sorted(c.items(), key=lambda kv: kv[0][1]) if mm == m} for m in METH.values()}
    kept = {str(g): {"true": sum(n for (_, hd), n in true.items() if hd <= g), "false": sum(n for (_, hd), n in false.items() if hd <= g)}
            for g in (30, 33, 36, 40, 44, 48, 174)}
    return {"snrs": snrs, "frames_per_snr": n_frames, "true_hd": hist(true), "false_hd": hist(false), "kept_by_gate": kept}


def timing(n_frames, reps):
    audio = synth.make_batch(0, n_frames)
    rxs = {"unset": Receiver("", None, max_frames=n_frames), "set": Receiver("", None, max_frames=n_frames, my_call=MY, dx_call=DX)}
    t = {k: [] for k in rxs}
    try:
        for rx in rxs.values():
            rx.decode_frames(audio)
        for _ in range(reps):
            for k, rx in rxs.items():
                t0 = time.perf_counter()
                rx.decode_frames(audio)
                t[k].append(time.perf_counter() - t0)
    finally:
        for rx in rxs.values():
            rx.close()
    return {k: {"median_ms": 1e3 * float(np.median(v)), "min_ms": 1e3 * float(np.min(v)), "max_ms": 1e3 * float(np.max(v))} for k, v in t.items()} | {"frames": n_frames, "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--noise-frames", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rate-frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--snrs", type=float, nargs="*", default=[-24.0, -23.0, -22.0, -21.0, -20.0, -19.0, -18.0])
    ap.add_argument("--out", default="profiles/ap_calls_measure.json")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "ap_max_hd_default": _lib.AP_MAX_HD_DEFAULT}
    out["noise"] = noise(a.noise_frames)
    print(json.dumps(out["noise"])[:2000], flush=True)
    out["workload_random_calls"] = workload_false(a.frames)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "hd_histogram"} for k, v in out["workload_random_calls"].items()}), flush=True)
    out["rate_vs_snr"] = rate_vs_snr(a.snrs, a.rate_frames)
    out["true_distances"] = true_distances([-21.0, -20.0, -19.0, -18.0], a.rate_frames)
    print(json.dumps(out["true_distances"]["kept_by_gate"]), flush=True)
    out["decode_frames_time"] = timing(a.frames, a.reps)
    print(json.dumps(out["decode_frames_time"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
