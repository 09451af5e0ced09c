"""Measurements behind the measured signal reports (ft8rx_set_reports) -> profiles/report_measure.json.

    python tools/report_measure.py cpu [out.json]     # the float64 twin against synthetic truth, 16 recipe frames (no GPU)
    python tools/report_measure.py gpu [out.json]     # one MI355X: k_report time per 256-frame config-1 batch, decode_frames with the
                                                      # setting off / on, the accuracy table of the 64-frame set next to the default
                                                      # fields' errors, the reports of the two fixture recordings (no ground truth)

Each part updates its own keys of the JSON file.  The recipe frames are those of tests/test_report.py."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "profiles", "report_measure.json")


def table(truth, got):
    """Errors of (snr dB, f Hz, t s) against truth, split at 0 dB of the true SNR as the tests split them."""
    truth, got = np.asarray(truth, float), np.asarray(got, float)
    e = got - truth
    lo = truth[:, 0] <= 0
    st = lambda x: dict(mean=float(x.mean()), std=float(x.std()), rms=float(np.sqrt((x ** 2).mean())), worst=float(np.abs(x).max()))
    return dict(n=len(e), n_le_0dB=int(lo.sum()), snr_le_0dB=st(e[lo, 0]), snr_gt_0dB=st(e[~lo, 0]), f_hz=st(e[:, 1]), t_s=st(e[:, 2]))


def cpu_part(res):
    import oracle as O
    from pyft8_amd import report as R
    from test_report import recipe_frame
    truth, got, dflt = [], [], []
    for i in range(16):
        audio, sig = recipe_frame(i)
        r = O.decode_frame(audio)
        spec = O.cycle_spectrum(audio)
        by_text = {s[4]: s for s in sig}
        for m in r["msgs"]:
            if m["msg_tuple"] not in by_text:
                continue
            w, f0, t0, snr, _ = by_text.pop(m["msg_tuple"])
            c = r["cands"][m["cand"]]
            tt, ft = (m["ttweak"], m["ftweak"]) if m["fine"] else (0, 0)
            x = R.measure(spec, c.f0_idx, c.h0_idx, tt, ft, w)
            truth.append((snr, f0, t0)); got.append((x["snr_db"], x["f_hz"], x["t_sec"])); dflt.append((m["snr"], m["fHz"], m["tsec"]))
    res["cpu_twin_16_frames"] = dict(report=table(truth, got), default_fields=table(truth, dflt))
    print(json.dumps(res["cpu_twin_16_frames"], indent=1))


def gpu_part(res):
    import torch  # noqa: F401 -- before libft8rx.so loads (_lib.lib)
    from pyft8_amd import _lib, synth
    from pyft8_amd.receiver import Receiver, frames_from_wav
    from test_report import recipe_frame
    # ---- k_report per 256-frame config-1 batch (stage times of a profiled batch), decodes per batch
    B = 256
    c1 = synth.make_batch(0, B)
    h = _lib.Handle(max_frames=B)
    h.set_reports(True)
    rec, cnt, ev, evc = h.decode_batch(c1)
    n_dec = int(sum((rec[f, :cnt[f]]["status"] == _lib.ST_DECODED).sum() for f in range(B)))
    h.set_profiling(True)
    times = []
    for _ in range(5):
        h.decode_batch(c1)
        h.sync()                                   # the stage times are taken there
        times.append({k: float(v) for k, v in h.stage_times().items()})
    h.close()
    rep_ms = sorted(t["report"] for t in times)
    res["k_report_config1"] = dict(frames=B, decodes_per_batch=n_dec, report_stage_ms_median_of_5=rep_ms[2], report_stage_ms_all=rep_ms,
                                   stage_ms_last_run=times[-1], us_per_decode=1e3 * rep_ms[2] / max(n_dec, 1))
    print("k_report", res["k_report_config1"], flush=True)
    # ---- decode_frames off / on: the median of 10 alternating runs
    rx = {False: Receiver("", None, max_frames=B), True: Receiver("", None, max_frames=B, reports=True)}
    for r in rx.values():
        r.decode_frames(c1)
    t = {False: [], True: []}
    for _ in range(10):
        for on in (False, True):
            t0 = time.perf_counter()
            rx[on].decode_frames(c1)
            t[on].append(1e3 * (time.perf_counter() - t0))
    for r in rx.values():
        r.close()
    res["decode_frames_256_config1_ms"] = dict(off_median=float(np.median(t[False])), on_median=float(np.median(t[True])), off=t[False], on=t[True])
    print("decode_frames", res["decode_frames_256_config1_ms"]["off_median"], res["decode_frames_256_config1_ms"]["on_median"], flush=True)
    # ---- accuracy on the 64-frame set, next to the default fields on the same messages
    frames = [recipe_frame(i) for i in range(16, 80)]
    audio = np.stack([f[0] for f in frames])
    r = Receiver("", None, max_frames=64, reports=True)
    d = r.decode_frames(audio)
    truth, got, dflt = [], [], []
    for f, (_, sig) in enumerate(frames):
        by_text = {s[4]: s for s in sig}
        for m in d[f]:
            if m["msg_tuple"] in by_text and m["report"] is not None:
                _, f0, t0, snr, _ = by_text.pop(m["msg_tuple"])
                truth.append((snr, f0, t0)); got.append((m["report"]["snr"], m["report"]["fHz"], m["report"]["tsec"]))
                dflt.append((int(m["their_snr"]), m["fHz"], m["tsec"]))
    res["gpu_64_frames"] = dict(report=table(truth, got), default_fields=table(truth, dflt))
    print("accuracy", json.dumps(res["gpu_64_frames"]), flush=True)
    # ---- the two fixture recordings: no ground truth exists, the reports are printed next to the default fields
    real = {}
    for wav in ("test_08.wav", "test_09.wav"):
        fr = frames_from_wav(os.path.join(ROOT, "tests", "golden", wav))
        real[wav] = [[dict(text=" ".join(m["msg_tuple"]), their_snr=m["their_snr"], fHz=m["fHz"], tsec=m["tsec"], report=m["report"]) for m in f]
                     for f in r.decode_frames(fr)]
    r.close()
    res["real_audio_no_ground_truth"] = real
    print("real audio:", {k: sum(map(len, v)) for k, v in real.items()}, "messages", flush=True)


def main():
    part = sys.argv[1] if len(sys.argv) > 1 else "cpu"
    res = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            res = json.load(f)
    (cpu_part if part == "cpu" else gpu_part)(res)
    out = sys.argv[2] if len(sys.argv) > 2 else OUT
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
