"""Measurements behind weak mode (ft8rx_set_weak) -> profiles/weak_measure.json.

    python tools/weak_measure.py cpu        # noise score distribution behind FT8RX_WEAK_SYNC_MIN_DEFAULT (numpy twin, no GPU)
    python tools/weak_measure.py gpu        # yield vs SNR, config 4, config-1 yield / rate / kernel times, noise false decodes,
                                            # OSD distance histograms behind FT8RX_WEAK_OSD_MAX_HD_DEFAULT (one MI355X)

Each part updates its own keys of the JSON file.  Frames: synth.frame_with_signals (10 signals >= 200 Hz apart, t0 in [0, 1.5] s) for
the SNR sweep, synth.make_frame for BASELINE configs 1 and 4, noise-only frame_with_signals(i, []) for false alarms."""
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "profiles", "weak_measure.json")
NOISE_SEED = 5_000_000
SENS_SEED = 6_000_000


def sens_frame(args):
    """One frame of the sensitivity set: 10 random messages 240 Hz apart (+-20 Hz), t0 uniform in [0, 1.5] s, all at snr dB."""
    from pyft8_amd import synth
    index, snr = args
    rng = np.random.default_rng(SENS_SEED + index)
    sig, truth = [], []
    for k in range(10):
        msg = synth.random_message(rng)
        f0 = 300.0 + 240.0 * k + rng.uniform(-20.0, 20.0)
        t0 = rng.uniform(0.0, 1.5)
        sig.append((synth.pack77(*msg), f0, t0, snr))
        truth.append((" ".join(msg), f0))
    return synth.frame_with_signals(SENS_SEED + index, sig), truth


def sens_set(n, snr, first=0):
    with mp.get_context("fork").Pool(16) as pool:
        r = pool.map(sens_frame, [(first + i, float(snr)) for i in range(n)])
    return np.stack([a for a, _ in r]), [t for _, t in r]


def noise_frame(i):
    from pyft8_amd import synth
    return synth.frame_with_signals(NOISE_SEED + i, [])


def noise_set(n):
    with mp.get_context("fork").Pool(16) as pool:
        return np.stack(pool.map(noise_frame, range(n)))


def _made(args):
    from pyft8_amd import synth
    i, nsig, lo, hi = args
    a, tr = synth.make_frame(i, n_signals=nsig, snr_range=(lo, hi), return_truth=True)
    return a, [(t["msg"], t["f0"]) for t in tr]


def made_set(start, n, nsig, snr):
    with mp.get_context("fork").Pool(16) as pool:
        r = pool.map(_made, [(start + i, nsig, snr[0], snr[1]) for i in range(n)])
    return np.stack([a for a, _ in r]), [t for _, t in r]


def score(dicts, truth):
    """(true, false) decodes: a message is true if its text is one of the frame's and its fHz within 10 Hz of that signal's f0."""
    t = f = 0
    for ms, tr in zip(dicts, truth):
        for m in ms:
            txt = " ".join(m["msg_tuple"])
            if any(txt == x and abs(m["fHz"] - f0) < 10 for x, f0 in tr):
                t += 1
            else:
                f += 1
    return t, f


def cpu_part(res, n=64):
    """Noise-only frames: per f0 bin the best score over h0 -- the reference's middle-block score and weak mode's three-block one."""
    import oracle as O
    import weak_twin as W
    frames = noise_set(n)
    ocfg = W.oracle_config()
    one, three = [], []
    f0 = np.arange(ocfg.f0_lo, ocfg.f0_hi)
    h0 = np.arange(ocfg.h0_lo, ocfg.h0_hi)
    for a in frames:
        g = O.spectrogram(a, ocfg)
        three.append(W.sync3_scores(g, ocfg.f0_lo, ocfg.f0_hi, ocfg.h0_lo, ocfg.h0_hi)[0])
        s1 = np.zeros((len(h0), len(f0)))
        ts = np.zeros_like(s1)
        for s in range(7):
            R = W._rows(g, h0 + 148 + 4 * s)
            t = np.zeros_like(s1)
            for k in range(14):
                t = t + R[:, f0 + k]
            ts = ts + t
            c = W.COSTAS[s]
            s1 = s1 + (R[:, f0 + 2 * c] + R[:, f0 + 2 * c + 1])
        one.append(np.maximum((s1 + W.W6 * (ts - s1)).astype(np.float32).max(axis=0), 0))
    one, three = np.concatenate(one), np.concatenate(three)
    rate85 = float((one > 85).mean())
    thr = float(np.quantile(three, 1.0 - rate85))
    res["noise_scores"] = dict(
        frames=n, bins=int(len(one)),
        one_block=dict(quantiles={str(q): float(np.quantile(one, q)) for q in (0.5, 0.9, 0.99, 0.999)},
                       frac_above_85=rate85, max=float(one.max())),
        three_block=dict(quantiles={str(q): float(np.quantile(three, q)) for q in (0.5, 0.9, 0.99, 0.999)},
                         frac_above={str(t): float((three > t).mean()) for t in (130, 140, 147, 155, 165)}, max=float(three.max())),
        three_block_threshold_at_the_reference_rate=thr)
    print(json.dumps(res["noise_scores"], indent=1))


def gpu_part(res, n_sens=32, n_noise=2048, n_c1=256, n_c4=2048):
    # every frame is made before the GPU is opened (forked generator processes)
    t0 = time.time()
    sweep = {snr: sens_set(n_sens, snr, first=1000 * (snr + 30)) for snr in range(-24, -15)}
    noise = noise_set(n_noise)
    c1, c1t = made_set(0, n_c1, 50, (-10.0, 10.0))
    c4, c4t = made_set(300000, n_c4, 10, (-24.0, -20.0))
    print(f"frames made in {time.time() - t0:.0f} s", flush=True)
    import torch  # noqa: F401 -- torch's HIP runtime serves both (_lib.lib)
    from pyft8_amd import _lib, messages
    from pyft8_amd.receiver import Receiver

    def run(frames, truth=None, **kw):
        rx = Receiver("", None, max_frames=min(len(frames), 512), **kw)
        out = []
        for i in range(0, len(frames), 512):
            out += rx.decode_frames(frames[i:i + 512])
        rx.close()
        if truth is None:
            return 0, sum(len(m) for m in out)
        return score(out, truth)

    res["snr_sweep"] = {"frames_per_point": n_sens, "signals_per_frame": 10}
    for snr, (fr, tr) in sweep.items():
        d, w = run(fr, tr), run(fr, tr, weak=True)
        res["snr_sweep"][str(snr)] = dict(default=dict(true=d[0], false=d[1]), weak=dict(true=w[0], false=w[1]))
        print("snr", snr, res["snr_sweep"][str(snr)], flush=True)
    d, w = run(noise), run(noise, weak=True)
    res["noise_false_decodes"] = dict(frames=n_noise, default=d[1], weak=w[1])
    print("noise", res["noise_false_decodes"], flush=True)
    d, w = run(c1, c1t), run(c1, c1t, weak=True)
    res["config1"] = dict(frames=n_c1, default=dict(true_per_frame=d[0] / n_c1, false_per_frame=d[1] / n_c1),
                          weak=dict(true_per_frame=w[0] / n_c1, false_per_frame=w[1] / n_c1))
    k4 = dict(osd_triple=30, osd_max_hd=32)
    d, w = run(c4, c4t, **k4), run(c4, c4t, weak=True, **k4)
    res["config4"] = dict(frames=n_c4, knobs=k4, default=dict(true_per_frame=d[0] / n_c4, false_per_frame=d[1] / n_c4),
                          weak=dict(true_per_frame=w[0] / n_c4, false_per_frame=w[1] / n_c4))
    print("c1", res["config1"], "c4", res["config4"], flush=True)
    # config-1 rate (host audio -> records, 256-frame batches) and the stage times of one profiled batch, default vs weak
    rate = {}
    for weak in (False, True):
        h = _lib.Handle(max_frames=n_c1)
        if weak:
            h.set_weak(True)
        h.decode_batch(c1)
        t = time.time()
        reps = 5
        for _ in range(reps):
            h.decode_batch(c1)
        fps = reps * n_c1 / (time.time() - t)
        h.set_profiling(True)
        h.decode_batch(c1)
        st = {k: float(v) for k, v in h.stage_times().items()} if isinstance(h.stage_times(), dict) else dict(zip(*h.stage_times()))
        h.close()
        rate["weak" if weak else "default"] = dict(frames_per_s=fps, stage_ms_per_256_frames=st)
    res["config1_rate"] = rate
    print("rate", rate, flush=True)
    # OSD distance histograms: weak mode with the gate open (osd_max_hd = 174), every OSD decode's distance, true vs false
    hist = dict(true={}, false={})
    sets = [sweep[-20], sweep[-19], sweep[-18], (noise[:512], [[] for _ in range(512)])]
    h = _lib.Handle(max_frames=512)
    h.set_weak(True, None, 174)
    for fr, tr in sets:
        rec, cnt, ev, evc = h.decode_batch(fr)
        msgs, mcnt = _lib.package_batch(rec, cnt, ev, evc)
        for f in range(len(fr)):
            for i, d in enumerate(messages.message_dicts(msgs[f], mcnt[f])):
                r = rec[f, int(msgs[f][i]["cand"])]
                if r["method"] not in (_lib.M_OSD, _lib.M_LDPC_B_OSD):
                    continue
                txt = " ".join(d["msg_tuple"])
                ok = any(txt == x and abs(d["fHz"] - f0) < 10 for x, f0 in tr[f])
                k = str(int(r["osd_hd"]))
                hist["true" if ok else "false"][k] = hist["true" if ok else "false"].get(k, 0) + 1
    h.close()
    res["osd_hd_histogram"] = dict(sets="sweep -20, -19, -18 dB + 512 noise frames; weak mode, osd_max_hd 174", **hist)
    print("hist", res["osd_hd_histogram"], flush=True)


def main():
    part = sys.argv[1] if len(sys.argv) > 1 else "cpu"
    res = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            res = json.load(f)
    if part == "cpu":
        cpu_part(res)
    else:
        gpu_part(res)
    out = sys.argv[2] if len(sys.argv) > 2 else OUT
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
