"""FT4 measurements on an MI355X -> profiles/ft4_measure.json; profiles/ft4_notes.md states what was seen.

    python tools/ft4_measure.py [--out profiles/ft4_measure.json] [--prob] [--noise] [--throughput] [--twin N] [--passes] [--coherent] [--weak]
                                [--coh-osd]
    python tools/ft4_measure.py --reports [--reports-twin] [--out profiles/ft4_report_measure.json]

--prob        decode probability against SNR: -20 .. -8 dB in 1-dB steps, 200 signals per step, 10 signals per frame (carriers >= 150 Hz
              apart, starts 0.1 .. 1.5 s), through Handle.ft4_decode and the native message layer; the 50 % point by interpolation
--noise       false decodes on 2048 noise-only frames for a sweep of the OSD distance gate (ft4_osd_max_hd), at msg_types 0 and all
--throughput  frames/s at B = 256 with 20 signals per frame (-14 .. +5 dB): 3 warm-up and 20 timed calls of ft4_decode (host frames, the
              copy included) and of ft4_enqueue + fetch (device-resident frames), the stage times (ft8rx_set_profiling)
--passes      subtraction passes (section 19.6) on 256 crowded frames (16 signals in 300 .. 1200 Hz, -12 .. +10 dB, make_frame indices 1000 ..
              1255): true and false decodes per frame for ft4_passes 1 / 2 / 3 at msg_types 0 (gate 40) and all (gate 24), the later
              passes' own gate (ft4_sub_osd_max_hd) swept, the times of one subtraction sweep and of a whole two-pass batch at B = 256
--coherent    coherent LLRs (section 19.8), each figure beside the same recipe with the setting off, on one handle in one session: decode
              probability at -19 .. -12 dB (the recipe of --prob) with the decodes by run length; false decodes on the 2048 noise frames
              at the default gates (40 at msg_types 0, 24 at all); frames/s at B = 256 with 20 signals per frame (device-resident), the
              stage times and the length of the list the coherent step works on
--weak        the weak search (section 19.10), each figure beside the same recipe with the setting off, in one session: the threshold
              that leaves the 2048 noise frames no more candidates than the default search leaves there at sync_min = 100 (both counted
              in this run); false decodes on those frames at that threshold, with ft4_coherent off and on, at gate 40 / msg_types 0 and
              gate 24 / all; decode probability at -18 .. -12 dB (the recipe of --prob) in four columns -- off, weak, coherent, weak +
              coherent -- with the truths that became candidates; frames/s at B = 256 with 20 signals per frame (device-resident),
              off / on alternating, twice each, and the stage times
--coh-osd     OSD on the coherent rows behind the whole-message score (section 19.11), in one session.  Collection, both gates open (max_hd 174,
              every score), weak search and coherent step on: (score, hd, run length, true or false) of every word the step returns on the
              candidates the chain leaves EXHAUSTED -- through the stage entries ft4_coherent, ft4_osd and ft4_verify, which make the
              chain's launches, so that the run-of-4 word is seen where a run-of-2 word would take precedence -- on the 2048 noise frames
              (msg_types 0 and all) and on the 200-signal sets at -18 .. -14 dB.  The two defaults from it: max_hd = the smallest multiple
              of 4 that keeps at least 99 % of the true words that score above the noise maximum; min_score = S_max + (S_max - S_90) of the
              noise words within that max_hd, rounded up to one decimal (for msg_types all from its own noise words).  Then, with those
              two: false decodes on the noise frames with weak on and off at msg_types 0 and all; the decode table at -18 .. -12 dB in the
              columns coherent, coherent + cosd, weak + coherent, weak + coherent + cosd with the decodes by run length and method; frames/s
              at B = 256 with 20 signals per frame, plain FT4 / coherent / coherent + cosd alternating, twice each, and the stage times
--reports     measured reports (section 19.9) -> profiles/ft4_report_measure.json: the accuracy recipe make_frame(i, n_signals=8, snr_range=
              (-14, 15), min_sep_hz=250) against truth, frames 16 .. 79 through Receiver(ft4_reports=True) with the default fields of the
              same messages beside it; the report stage timed with HIP events (ft8rx_set_profiling) at B = 256 with 20 signals per frame;
              decode_frames_ft4 with the setting off and on in paired alternating runs
--reports-twin  no GPU: frames 0 .. 15 of the same recipe through decode_twin and the twin's report, into the same file
--twin N      no GPU: the yardstick, the float64 twin with the numpy BP on N signals per step of -18 .. -11 dB (the same recipe)
Results are merged into the file's existing sections."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyft8_amd import ft4  # noqa: E402

PROB_SNRS = list(range(-20, -7))
GATES = [16, 20, 24, 28, 30, 32, 36, 40, 48, 174]


def prob_frame(step, k, snr):
    return ft4.make_frame(100000 + 1000 * (step + 40) + k, n_signals=10, snr_range=(snr, snr), return_truth=True)


def half_point(snrs, p):
    for a, b, pa, pb in zip(snrs, snrs[1:], p, p[1:]):
        if pa < 0.5 <= pb:
            return a + (0.5 - pa) / (pb - pa) * (b - a)
    return None


def texts_of(h, res, mask=0):
    from pyft8_amd import _lib
    msgs, cnt = (_lib.package_batch_ext(*res, mask) if mask else _lib.package_batch(*res))[:2]
    return [{" ".join(x.decode() for x in m["f"].tolist()).strip() for m in msgs[f][:cnt[f]]} for f in range(len(cnt))]


def measure_prob(h, per_step=200):
    out = {"snr_db": PROB_SNRS, "signals_per_step": per_step, "decoded": [], "bp": [], "osd": []}
    for snr in PROB_SNRS:
        frames = [prob_frame(snr, k, float(snr)) for k in range(per_step // 10)]
        res = h.ft4_decode(np.stack([f[0] for f in frames]))
        got = texts_of(h, res)
        n = sum(t["msg"] in got[f] for f, (_, truth) in enumerate(frames) for t in truth)
        rec, cnt = res[0], res[1]
        dec = np.concatenate([rec[f, :cnt[f]] for f in range(len(cnt))])
        dec = dec[dec["status"] == 1]
        out["decoded"].append(n); out["bp"].append(int((dec["ipass"] == 4).sum())); out["osd"].append(int((dec["ipass"] == 5).sum()))
        print(f"prob {snr:+d} dB: {n}/{per_step}", flush=True)
    p = [d / per_step for d in out["decoded"]]
    out["probability"] = p
    out["half_point_db"] = half_point(PROB_SNRS, p)
    return out


def measure_twin(per_step):
    snrs = list(range(-18, -10))
    out = {"snr_db": snrs, "signals_per_step": per_step, "decoded": []}
    for snr in snrs:
        n = 0
        for k in range((per_step + 9) // 10):
            x, truth = prob_frame(snr, k, float(snr))
            words = {c["word"] for c in ft4.decode_twin(x) if c["word"] is not None}
            n += sum(t["word"] in words for t in truth[:min(10, per_step - 10 * k)])
        out["decoded"].append(n)
        print(f"twin {snr:+d} dB: {n}/{per_step}", flush=True)
    p = [d / per_step for d in out["decoded"]]
    out["probability"] = p
    out["half_point_db"] = half_point(snrs, p)
    return out


def noise_frames(n, first):
    rng = np.random.Generator(np.random.Philox(key=ft4.SEED_BASE + 7000000 + first))
    return np.clip(np.rint(rng.standard_normal((n, ft4.NFRAME)) * 1000.0), -32768, 32767).astype(np.int16)


def measure_noise(h, n_frames=2048, chunk=256):
    from pyft8_amd import _lib
    out = {"frames": n_frames, "gates": GATES, "false_decodes": {"0": [0] * len(GATES), "all": [0] * len(GATES)}, "candidates": 0, "texts": []}
    for first in range(0, n_frames, chunk):
        a = noise_frames(chunk, first)
        for name, mask in (("0", 0), ("all", _lib.MT_ALL)):
            h.set_msg_types(mask)
            for g, gate in enumerate(GATES):
                h.ft4_set(osd_max_hd=gate)
                res = h.ft4_decode(a)
                rec, cnt = res[0], res[1]
                if g == 0 and mask == 0:
                    out["candidates"] += int(cnt.sum())
                k = sum(int((rec[f, :cnt[f]]["status"] == 1).sum()) for f in range(chunk))
                out["false_decodes"][name][g] += k
                if k:
                    out["texts"] += [f"gate {gate} mask {name}: {t}" for s in texts_of(h, res, mask) for t in s][:4]
        print(f"noise frames {first + chunk}: {out['false_decodes']}", flush=True)
    h.set_msg_types(0)
    h.ft4_set()
    out["texts"] = out["texts"][:40]
    return out


def throughput_frame(k, n_signals=20):
    """20 standard messages, carriers 140 Hz apart from 200 Hz on (+- 20 Hz), starts 0.1 .. 1.5 s, -14 .. +5 dB"""
    rng = np.random.Generator(np.random.Philox(key=ft4.SEED_BASE + 200000 + k))
    sigs = [(ft4.pack77(*ft4.random_message(rng)), 200.0 + 140.0 * i + rng.uniform(-20.0, 20.0), rng.uniform(0.1, 1.5), rng.uniform(-14.0, 5.0))
            for i in range(n_signals)]
    return ft4.frame_with_signals(200000 + k, sigs)


def measure_throughput(h, B=256, warmup=3, steps=20):
    import torch
    a = np.stack([throughput_frame(k) for k in range(B)])
    out = {"B": B, "signals_per_frame": 20, "warmup": warmup, "steps": steps}
    for _ in range(warmup):
        res = h.ft4_decode(a)
    t = []
    for _ in range(steps):
        t0 = time.perf_counter(); res = h.ft4_decode(a); t.append(time.perf_counter() - t0)
    out["host_frames_per_s"] = B / float(np.median(t)); out["host_step_ms"] = [round(1e3 * x, 3) for x in t]
    out["decoded_per_frame"] = float(sum(int((res[0][f, :res[1][f]]["status"] == 1).sum()) for f in range(B))) / B
    d = torch.from_numpy(a).to("cuda:0"); torch.cuda.synchronize()
    for _ in range(warmup):
        h.ft4_enqueue(d.data_ptr(), B); h.fetch(B)
    t = []
    for _ in range(steps):
        t0 = time.perf_counter(); h.ft4_enqueue(d.data_ptr(), B); h.fetch(B); t.append(time.perf_counter() - t0)
    out["device_frames_per_s"] = B / float(np.median(t)); out["device_step_ms"] = [round(1e3 * x, 3) for x in t]
    h.set_profiling(True)
    h.ft4_enqueue(d.data_ptr(), B); h.fetch(B); h.sync()
    out["stage_ms"] = {k: round(float(v), 4) for k, v in h.stage_times().items()}
    h.set_profiling(False)
    print("throughput", out["host_frames_per_s"], out["device_frames_per_s"], out["stage_ms"], flush=True)
    return out


def measure_coherent(h, noise_frames_n=2048, chunk=256, per_step=200, B=256, warmup=3, steps=20):
    import torch
    from pyft8_amd import _lib
    snrs = list(range(-19, -11))
    out = {"probability": {"snr_db": snrs, "signals_per_step": per_step}, "noise": {"frames": noise_frames_n}, "throughput": {"B": B, "signals_per_frame": 20}}
    live = lambda res: np.concatenate([res[0][f, :res[1][f]] for f in range(len(res[1]))])
    # ---- decode probability
    for name, on in (("off", False), ("on", True)):
        h.ft4_set_coherent(on)
        r = {"decoded": [], "bp": [], "runs_of_2": [], "runs_of_4": [], "osd": []}
        for snr in snrs:
            frames = [prob_frame(snr, k, float(snr)) for k in range(per_step // 10)]
            res = h.ft4_decode(np.stack([f[0] for f in frames]))
            got = texts_of(h, res)
            r["decoded"].append(sum(t["msg"] in got[f] for f, (_, truth) in enumerate(frames) for t in truth))
            dec = live(res); dec = dec[dec["status"] == 1]
            r["bp"].append(int(((dec["ipass"] == 4) & (dec["nsync"] == 0)).sum())); r["osd"].append(int((dec["ipass"] == 5).sum()))
            r["runs_of_2"].append(int((dec["nsync"] == 2).sum())); r["runs_of_4"].append(int((dec["nsync"] == 4).sum()))
            print(f"coherent {name} prob {snr:+d} dB: {r['decoded'][-1]}/{per_step}", flush=True)
        r["probability"] = [d / per_step for d in r["decoded"]]
        r["half_point_db"] = half_point(snrs, r["probability"])
        out["probability"][name] = r
    # ---- false decodes on noise, the default gates
    nz = {f"{name}_{m}": {"false_decodes": 0, "by_run_length": {"1": 0, "2": 0, "4": 0, "osd": 0}, "texts": []} for name in ("off", "on") for m in ("0", "all")}
    cands = 0
    for first in range(0, noise_frames_n, chunk):
        a = noise_frames(chunk, first)
        for m, mask, gate in (("0", 0, ft4.OSD_MAX_HD_DEFAULT), ("all", _lib.MT_ALL, ft4.OSD_MAX_HD_MSG_TYPES)):
            h.set_msg_types(mask); h.ft4_set(osd_max_hd=gate)
            for name, on in (("off", False), ("on", True)):
                h.ft4_set_coherent(on)
                res = h.ft4_decode(a)
                if m == "0" and not on:
                    cands += int(res[1].sum())
                dec = live(res); dec = dec[dec["status"] == 1]
                e = nz[f"{name}_{m}"]
                e["false_decodes"] += len(dec)
                for x in dec:
                    e["by_run_length"]["osd" if x["ipass"] == 5 else str(int(x["nsync"]) or 1)] += 1
                if len(dec):
                    e["texts"] += [f"frame {first + f}: {t}" for f, s in enumerate(texts_of(h, res, mask)) for t in s]
        print(f"coherent noise frames {first + chunk}: " + ", ".join(f"{k} {v['false_decodes']}" for k, v in nz.items()), flush=True)
    h.set_msg_types(0); h.ft4_set()
    out["noise"].update(nz); out["noise"]["candidates"] = cands
    # ---- throughput, device-resident frames
    a = np.stack([throughput_frame(k) for k in range(B)])
    d = torch.from_numpy(a).to("cuda:0"); torch.cuda.synchronize()
    for name, on in (("off", False), ("on", True), ("off_again", False), ("on_again", True)):
        h.ft4_set_coherent(on)
        for _ in range(warmup):
            h.ft4_enqueue(d.data_ptr(), B); res = h.fetch(B)
        t = []
        for _ in range(steps):
            t0 = time.perf_counter(); h.ft4_enqueue(d.data_ptr(), B); res = h.fetch(B); t.append(time.perf_counter() - t0)
        rec = live(res); dec = rec[rec["status"] == 1]
        first_bp = int(((dec["ipass"] == 4) & (dec["nsync"] == 0)).sum())
        h.set_profiling(True)
        h.ft4_enqueue(d.data_ptr(), B); h.fetch(B); h.sync()
        stage = {k: round(float(v), 4) for k, v in h.stage_times().items()}
        h.set_profiling(False)
        out["throughput"][name] = {"device_frames_per_s": B / float(np.median(t)), "device_step_ms": [round(1e3 * x, 3) for x in t], "stage_ms": stage,
                                   "candidates": len(rec), "decoded": len(dec), "list_behind_first_bp": len(rec) - first_bp,
                                   "runs_of_2": int((dec["nsync"] == 2).sum()), "runs_of_4": int((dec["nsync"] == 4).sum()), "osd": int((dec["ipass"] == 5).sum())}
        print("coherent throughput", name, out["throughput"][name]["device_frames_per_s"], stage, flush=True)
    h.ft4_set_coherent(False)
    return out


def weak_kept(best):
    """best [B][nf0] -> the scores of the bins k_ft4_peaks keeps at any threshold: no lower neighbour at or above, no higher one above"""
    b = np.asarray(best, np.float64)
    left = np.concatenate([np.full((len(b), 1), -np.inf), b[:, :-1]], axis=1)
    right = np.concatenate([b[:, 1:], np.full((len(b), 1), -np.inf)], axis=1)
    return b[(left < b) & (right <= b)]


def found_as_candidates(res, frames):
    """truths with a candidate within 1 bin and 2.5 rows"""
    n = 0
    for f, (_, truth) in enumerate(frames):
        r = res[0][f, :res[1][f]]
        for t in truth:
            n += bool(np.any((np.abs(r["f0_idx"] - t["f0"] / ft4.BIN_HZ) <= 1) & (np.abs(r["h0_idx"] - t["t0"] * ft4.FS / ft4.HOP) <= 2.5)))
    return n


def measure_weak(h, noise_frames_n=2048, chunk=256, per_step=200, B=256, warmup=3, steps=20):
    import torch
    from pyft8_amd import _lib
    snrs = list(range(-18, -11))
    out = {"threshold": {"frames": noise_frames_n}, "noise": {"frames": noise_frames_n}, "probability": {"snr_db": snrs, "signals_per_step": per_step},
           "throughput": {"B": B, "signals_per_frame": 20}}
    live = lambda res: np.concatenate([res[0][f, :res[1][f]] for f in range(len(res[1]))])

    def setting(weak, coh, weak_min=None):
        h.ft4_set_weak(weak, weak_min); h.ft4_set_coherent(coh)
    # ---- the threshold: the default search's candidates on the noise frames, and the weak search's kept maxima there
    yard, kept = 0, []
    for first in range(0, noise_frames_n, chunk):
        a = noise_frames(chunk, first)
        setting(False, False)
        yard += int(h.ft4_decode(a)[1].sum())
        kept.append(weak_kept(h.ft4_sync_weak(a, want_best=True)[4]))
    kept = np.sort(np.concatenate(kept))[::-1]
    # the smallest threshold, to two decimals, with no more than `yard` kept maxima at or above it (float32 scores against a float32 cut)
    t = np.ceil(float(kept[yard]) * 100.0) / 100.0 if yard < len(kept) else 0.01
    while int((kept >= np.float32(t)).sum()) > yard:
        t = round(t + 0.01, 2)
    out["threshold"].update(default_search_candidates=yard, weak_min=t, weak_candidates_at_it=int((kept >= np.float32(t)).sum()),
                            kept_maxima=len(kept), highest=[round(float(v), 3) for v in kept[:8]],
                            candidates_per_frame_at={f"{c:.2f}": float((kept >= np.float32(c)).sum()) / noise_frames_n for c in (15.0, 15.25, 15.5, 15.75, 16.0, 16.25, 16.5)})
    print("weak threshold", out["threshold"], flush=True)
    wm = t
    # ---- false decodes on noise at that threshold, the default gates
    cols = (("off", False, False), ("weak", True, False), ("coherent", False, True), ("weak_coherent", True, True))
    nz = {f"{name}_{m}": {"false_decodes": 0, "candidates": 0, "texts": []} for name, _, _ in cols for m in ("0", "all")}
    for first in range(0, noise_frames_n, chunk):
        a = noise_frames(chunk, first)
        for m, mask, gate in (("0", 0, ft4.OSD_MAX_HD_DEFAULT), ("all", _lib.MT_ALL, ft4.OSD_MAX_HD_MSG_TYPES)):
            h.set_msg_types(mask); h.ft4_set(osd_max_hd=gate)
            for name, weak, coh in cols:
                setting(weak, coh, wm)
                res = h.ft4_decode(a)
                dec = live(res); dec = dec[dec["status"] == 1]
                e = nz[f"{name}_{m}"]
                e["false_decodes"] += len(dec); e["candidates"] += int(res[1].sum())
                if len(dec):
                    e["texts"] += [f"frame {first + f}: {t}" for f, s in enumerate(texts_of(h, res, mask)) for t in s]
        print(f"weak noise frames {first + chunk}: " + ", ".join(f"{k} {v['false_decodes']}/{v['candidates']}" for k, v in nz.items()), flush=True)
    h.set_msg_types(0); h.ft4_set()
    out["noise"].update(nz); out["noise"]["weak_min"] = wm
    # ---- decode probability, four columns
    for name, weak, coh in cols:
        setting(weak, coh, wm)
        r = {"decoded": [], "candidates": [], "truths_as_candidates": []}
        for snr in snrs:
            frames = [prob_frame(snr, k, float(snr)) for k in range(per_step // 10)]
            res = h.ft4_decode(np.stack([f[0] for f in frames]))
            got = texts_of(h, res)
            r["decoded"].append(sum(t["msg"] in got[f] for f, (_, truth) in enumerate(frames) for t in truth))
            r["candidates"].append(int(res[1].sum())); r["truths_as_candidates"].append(found_as_candidates(res, frames))
            print(f"weak {name} prob {snr:+d} dB: {r['decoded'][-1]}/{per_step}, {r['truths_as_candidates'][-1]} truths among {r['candidates'][-1]} candidates", flush=True)
        r["probability"] = [d / per_step for d in r["decoded"]]
        r["half_point_db"] = half_point(snrs, r["probability"])
        out["probability"][name] = r
    # ---- throughput, device-resident frames
    a = np.stack([throughput_frame(k) for k in range(B)])
    d = torch.from_numpy(a).to("cuda:0"); torch.cuda.synchronize()
    for name, weak in (("off", False), ("on", True), ("off_again", False), ("on_again", True)):
        setting(weak, False, wm)
        for _ in range(warmup):
            h.ft4_enqueue(d.data_ptr(), B); res = h.fetch(B)
        tt = []
        for _ in range(steps):
            t0 = time.perf_counter(); h.ft4_enqueue(d.data_ptr(), B); res = h.fetch(B); tt.append(time.perf_counter() - t0)
        rec = live(res)
        h.set_profiling(True)
        h.ft4_enqueue(d.data_ptr(), B); h.fetch(B); h.sync()
        stage = {k: round(float(v), 4) for k, v in h.stage_times().items()}
        h.set_profiling(False)
        out["throughput"][name] = {"device_frames_per_s": B / float(np.median(tt)), "device_step_ms": [round(1e3 * x, 3) for x in tt], "stage_ms": stage,
                                   "candidates": len(rec), "decoded": int((rec["status"] == 1).sum())}
        print("weak throughput", name, out["throughput"][name]["device_frames_per_s"], stage, flush=True)
    out["throughput"]["workspace_bytes"] = h.ft4_weak_info()["workspace_bytes"]
    setting(False, False)
    return out


def cosd_words(h, a, res, mask, truth_words=None):
    """Every word the step returns on the candidates the batch `res` of frames `a` left EXHAUSTED, gates open: rows of (frame, score, hd,
    run length, true) -- true = the word is among the frame's planted ones (never on noise)"""
    from pyft8_amd import _lib
    rec, cnt = res[0], res[1]
    fr, idx = [], []
    for f in range(len(cnt)):
        k = np.nonzero(rec[f, :cnt[f]]["status"] == _lib.ST_EXHAUSTED)[0]
        fr += [f] * len(k); idx += list(k)
    if not fr:
        return []
    r = rec[fr, idx]
    pos = [r[k].astype(np.int32) for k in ("f0_idx", "h0_idx", "ttweak", "ftweak")]
    c = h.ft4_coherent(a, fr, *pos)
    rows = []
    for L, key in ((2, "llr2"), (4, "llr4")):
        ok, lo, hi, _, hd = h.ft4_osd(c[key], h.cfg.osd_single, h.cfg.osd_double, h.cfg.osd_triple, 174, mask)
        words = [(int(b) << 64) | int(x) if o else 0 for o, x, b in zip(ok, lo, hi)]
        sc = h.ft4_verify(a, fr, *pos, c["q"], words)
        rows += [(fr[i], float(sc[i]), int(hd[i]), L, bool(truth_words is not None and words[i] in truth_words[fr[i]])) for i in range(len(fr)) if ok[i]]
    return rows


def cosd_defaults(true_rows, noise_rows):
    """(max_hd, min_score, figures) by the rule of --coh-osd from rows of (frame, score, hd, run length, true)"""
    ns = np.array([r[1] for r in noise_rows]); nh = np.array([r[2] for r in noise_rows])
    ts = np.array([r[1] for r in true_rows]); th = np.array([r[2] for r in true_rows])
    top = float(ns.max())
    good = th[ts > top]
    max_hd = next(m for m in range(4, 180, 4) if (good <= m).sum() >= 0.99 * len(good))
    inside = np.sort(ns[nh <= max_hd])
    s_max, s_90 = float(inside[-1]), float(np.percentile(inside, 90))
    min_score = float(np.ceil((s_max + (s_max - s_90)) * 10.0 - 1e-9) / 10.0)
    return max_hd, min_score, {"noise_words": len(ns), "noise_max": top, "true_words": len(ts), "true_above_noise_max": len(good),
                               "true_above_hd": [int(good.min()), int(good.max())] if len(good) else None, "noise_words_within_max_hd": len(inside),
                               "s_max": s_max, "s_90": s_90}


def measure_coh_osd(h, noise_frames_n=2048, chunk=256, per_step=200, B=256, warmup=3, steps=20):
    import torch
    from pyft8_amd import _lib
    out = {"collection": {"frames": noise_frames_n, "max_hd": 174}, "noise": {"frames": noise_frames_n},
           "probability": {"snr_db": list(range(-18, -11)), "signals_per_step": per_step}, "throughput": {"B": B, "signals_per_frame": 20}}
    live = lambda res: np.concatenate([res[0][f, :res[1][f]] for f in range(len(res[1]))])
    masks = (("0", 0, ft4.OSD_MAX_HD_DEFAULT), ("all", _lib.MT_ALL, ft4.OSD_MAX_HD_MSG_TYPES))

    def setting(weak, coh, cosd, min_score=None, max_hd=None):
        h.ft4_set_weak(weak); h.ft4_set_coherent(coh); h.ft4_set_coh_osd(cosd, min_score, max_hd)
    # ---- collection: noise at both masks, then the signal sets -- with the weak search (the recipe) and, pooled with it, with the
    # default search: its candidates are other ones, and the step runs behind either
    noise = {"0": [], "all": []}
    weak_only = {"0": [], "all": []}
    for first in range(0, noise_frames_n, chunk):
        a = noise_frames(chunk, first)
        for m, mask, gate in masks:
            h.set_msg_types(mask); h.ft4_set(osd_max_hd=gate)
            for weak in (True, False):
                setting(weak, True, False)
                rows = [(first + r[0],) + r[1:] for r in cosd_words(h, a, h.ft4_decode(a), mask)]
                noise[m] += rows
                if weak:
                    weak_only[m] += rows
        print(f"coh-osd collection, noise frames {first + chunk}: {len(noise['0'])} / {len(noise['all'])} words ({len(weak_only['0'])} / {len(weak_only['all'])} behind the weak search)", flush=True)
    h.set_msg_types(0); h.ft4_set()
    sig, sig_weak = {}, []
    for snr in range(-18, -13):
        frames = [prob_frame(snr, k, float(snr)) for k in range(per_step // 10)]
        a = np.stack([f[0] for f in frames])
        sig[str(snr)] = []
        for weak in (True, False):
            setting(weak, True, False)
            rows = cosd_words(h, a, h.ft4_decode(a), 0, [{t["word"] for t in truth} for _, truth in frames])
            sig[str(snr)] += rows
            if weak:
                sig_weak += rows
        tr = [r for r in sig[str(snr)] if r[4]]
        print(f"coh-osd collection {snr:+d} dB: {len(sig[str(snr)])} words, {len(tr)} true (scores {min((r[1] for r in tr), default=0):.1f} .. {max((r[1] for r in tr), default=0):.1f})", flush=True)
    true_rows = [r for rows in sig.values() for r in rows if r[4]]
    false_rows = [r for rows in sig.values() for r in rows if not r[4]]
    recipe = {m: cosd_defaults([r for r in sig_weak if r[4]], weak_only[m]) for m in weak_only}      # the weak search alone
    out["collection"]["weak_search_alone"] = {m: {"max_hd": v[0], "min_score": v[1], **v[2]} for m, v in recipe.items()}
    max_hd, min_score, fig = cosd_defaults(true_rows, noise["0"])
    _, min_score_all, fig_all = cosd_defaults(true_rows, noise["all"])
    q = lambda v: [round(float(x), 2) for x in np.percentile(v, [0, 10, 50, 90, 99, 100])] if len(v) else None
    out["collection"].update(
        max_hd_default=max_hd, min_score_default=min_score, min_score_msg_types_all=min_score_all, msg_types_0=fig, msg_types_all=fig_all,
        noise_score_percentiles_0_10_50_90_99_100={m: q([r[1] for r in noise[m]]) for m in noise},
        noise_hd_percentiles={m: q([r[2] for r in noise[m]]) for m in noise},
        noise_top={m: sorted(((round(r[1], 2), r[2], r[3]) for r in noise[m]), reverse=True)[:12] for m in noise},
        true_by_snr={k: {"words": len([r for r in v if r[4]]), "score": q([r[1] for r in v if r[4]]), "hd": q([r[2] for r in v if r[4]]),
                         "above_min_score_within_max_hd": len([r for r in v if r[4] and r[1] >= min_score and r[2] <= max_hd])} for k, v in sig.items()},
        wrong_words_on_signal_frames={"words": len(false_rows), "score": q([r[1] for r in false_rows]),
                                      "above_min_score_within_max_hd": len([r for r in false_rows if r[1] >= min_score and r[2] <= max_hd])})
    print("coh-osd defaults", max_hd, min_score, min_score_all, fig, fig_all, flush=True)
    # ---- false decodes on the noise frames with the two defaults
    nz = {f"{w}_{m}": {"false_decodes": 0, "candidates": 0, "texts": []} for w in ("weak_off", "weak_on") for m in ("0", "all")}
    for first in range(0, noise_frames_n, chunk):
        a = noise_frames(chunk, first)
        for m, mask, gate in masks:
            h.set_msg_types(mask); h.ft4_set(osd_max_hd=gate)
            for w, weak in (("weak_off", False), ("weak_on", True)):
                setting(weak, True, True, min_score_all if mask else min_score, max_hd)
                res = h.ft4_decode(a)
                dec = live(res); dec = dec[dec["status"] == 1]
                e = nz[f"{w}_{m}"]
                e["false_decodes"] += len(dec); e["candidates"] += int(res[1].sum())
                if len(dec):
                    e["texts"] += [f"frame {first + f}: {t}" for f, s in enumerate(texts_of(h, res, mask)) for t in s]
        print(f"coh-osd noise frames {first + chunk}: " + ", ".join(f"{k} {v['false_decodes']}/{v['candidates']}" for k, v in nz.items()), flush=True)
    h.set_msg_types(0); h.ft4_set()
    out["noise"].update(nz); out["noise"].update(min_score=min_score, min_score_all=min_score_all, max_hd=max_hd)
    # ---- the decode table
    for name, weak, cosd in (("coherent", False, False), ("coherent_cosd", False, True), ("weak_coherent", True, False), ("weak_coherent_cosd", True, True)):
        setting(weak, True, cosd, min_score, max_hd)
        r = {"decoded": [], "false": [], "bp_1": [], "bp_2": [], "bp_4": [], "osd_1": [], "osd_2": [], "osd_4": []}
        for snr in out["probability"]["snr_db"]:
            frames = [prob_frame(snr, k, float(snr)) for k in range(per_step // 10)]
            res = h.ft4_decode(np.stack([f[0] for f in frames]))
            got = texts_of(h, res)
            r["decoded"].append(sum(t["msg"] in got[f] for f, (_, truth) in enumerate(frames) for t in truth))
            r["false"].append(sum(len(got[f] - {t["msg"] for t in truth}) for f, (_, truth) in enumerate(frames)))
            dec = live(res); dec = dec[dec["status"] == 1]
            for ip, meth in ((4, "bp"), (5, "osd")):
                for L in (1, 2, 4):
                    r[f"{meth}_{L}"].append(int(((dec["ipass"] == ip) & (dec["nsync"] == (0 if L == 1 else L))).sum()))
            print(f"coh-osd {name} prob {snr:+d} dB: {r['decoded'][-1]}/{per_step}, false {r['false'][-1]}", flush=True)
        r["probability"] = [d / per_step for d in r["decoded"]]
        r["half_point_db"] = half_point(out["probability"]["snr_db"], r["probability"])
        out["probability"][name] = r
    # ---- throughput, device-resident frames
    a = np.stack([throughput_frame(k) for k in range(B)])
    d = torch.from_numpy(a).to("cuda:0"); torch.cuda.synchronize()
    for name, coh, cosd in (("plain", False, False), ("coherent", True, False), ("coherent_cosd", True, True),
                            ("plain_again", False, False), ("coherent_again", True, False), ("coherent_cosd_again", True, True)):
        setting(False, coh, cosd, min_score, max_hd)
        for _ in range(warmup):
            h.ft4_enqueue(d.data_ptr(), B); res = h.fetch(B)
        tt = []
        for _ in range(steps):
            t0 = time.perf_counter(); h.ft4_enqueue(d.data_ptr(), B); res = h.fetch(B); tt.append(time.perf_counter() - t0)
        rec = live(res); dec = rec[rec["status"] == 1]
        h.set_profiling(True)
        h.ft4_enqueue(d.data_ptr(), B); h.fetch(B); h.sync()
        stage = {k: round(float(v), 4) for k, v in h.stage_times().items()}
        h.set_profiling(False)
        out["throughput"][name] = {"device_frames_per_s": B / float(np.median(tt)), "device_step_ms": [round(1e3 * x, 3) for x in tt], "stage_ms": stage,
                                   "candidates": len(rec), "decoded": len(dec), "cosd_decodes": int(((dec["ipass"] == 5) & (dec["nsync"] != 0)).sum())}
        print("coh-osd throughput", name, out["throughput"][name]["device_frames_per_s"], stage, flush=True)
    out["throughput"]["workspace_bytes"] = h.ft4_coh_osd_info()["workspace_bytes"]
    setting(False, False, False)
    return out


CROWDED_KW = dict(n_signals=16, snr_range=(-12, 10), freq_range=(300, 1200), t0_range=(0.2, 1.2), min_sep_hz=25)
SUB_GATES = [None, 32, 24, 16]


def measure_passes(B=256, first=1000):
    import torch
    from pyft8_amd import _lib
    from pyft8_amd.receiver import Receiver
    frames = [ft4.make_frame(first + k, return_truth=True, **CROWDED_KW) for k in range(B)]
    audio = np.stack([f[0] for f in frames])
    planted = [{t["msg"] for t in f[1]} for f in frames]
    out = {"frames": B, "first_index": first, "recipe": {k: list(v) if isinstance(v, tuple) else v for k, v in CROWDED_KW.items()}, "signals": 16 * B, "yield": {}}
    for name, kw in (("msg_types_0", {}), ("msg_types_all", {"msg_types": "all"})):
        for gate in SUB_GATES:
            for p in (1, 2, 3):
                if p == 1 and gate is not None:
                    continue
                r = Receiver("", None, max_frames=B, ft4_passes=p, ft4_sub_osd_max_hd=gate, **kw)
                t0 = time.perf_counter()
                res = r.decode_frames_ft4(audio)
                dt = time.perf_counter() - t0
                r.close()
                texts = [[" ".join(x for x in d["msg_tuple"] if x) for d in fr] for fr in res]
                true = sum(t in planted[f] for f in range(B) for t in texts[f])
                false = [(f, t, d["decode_notes"]) for f in range(B) for t, d in zip(texts[f], res[f]) if t not in planted[f]]
                sub = [d for fr in res for d in fr if "_SUB" in d["decode_notes"]]
                key = f"passes_{p}" + ("" if gate is None else f"_sub_gate_{gate}")
                out["yield"].setdefault(name, {})[key] = {
                    "true_per_frame": true / B, "false_per_frame": len(false) / B, "true": true, "false": len(false),
                    "false_in_later_passes": sum("_SUB" in n for _, _, n in false), "later_pass_decodes": len(sub),
                    "later_pass_osd": sum("OSD" in d["decode_notes"] for d in sub), "false_texts": [f"frame {first + f}: {t} ({n})" for f, t, n in false][:12],
                    "first_call_seconds": round(dt, 3)}
                print(name, key, out["yield"][name][key], flush=True)
    # times at B = 256: pass 1, the list, one sweep (synchronous call, a fresh device copy each time), the second pass; then whole batches
    h = _lib.Handle(max_frames=B)
    res = h.ft4_decode(audio)
    sigs = _lib.ft4_subtraction_list(res[0], res[1])
    t = {"sweep_ms": [], "signals_in_sweep": int(sigs[1].sum()), "longest_list": int(sigs[1].max())}
    for _ in range(6):
        d = torch.from_numpy(audio).to("cuda:0"); torch.cuda.synchronize()
        t0 = time.perf_counter(); h.ft4_subtract(d.data_ptr(), B, sigs, refine=1); t["sweep_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
    t0 = time.perf_counter(); h.ft4_subtract(d.data_ptr(), B, sigs, refine=0); t["sweep_refine0_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    h.close()
    for p in (1, 2, 3):
        r = Receiver("", None, max_frames=B, ft4_passes=p)
        r.decode_frames_ft4(audio)
        tt = []
        for _ in range(5):
            t0 = time.perf_counter(); r.decode_frames_ft4(audio); tt.append(round(1e3 * (time.perf_counter() - t0), 3))
        r.close()
        t[f"receiver_passes_{p}_ms"] = tt
    out["times"] = t
    print("times", t, flush=True)
    return out


REPORT_RECIPE = dict(n_signals=8, snr_range=(-14, 15), min_sep_hz=250, return_truth=True)


def report_recipe_frames(indices):
    """-> [(index, frame, truth)] and the indices where eight carriers 250 Hz apart do not fit make_frame's default band"""
    made, missing = [], []
    for i in indices:
        try:
            x, truth = ft4.make_frame(i, **REPORT_RECIPE)
            made.append((i, x, truth))
        except ValueError:
            missing.append(i)
    return made, missing


def report_stats(rows):
    """rows of (truth snr, snr error dB, frequency error Hz, time error ms)"""
    e = np.asarray(rows, np.float64).reshape(-1, 4)
    out = {}
    for name, m in (("snr_le_0", e[:, 0] <= 0.0), ("snr_gt_0", e[:, 0] > 0.0), ("all", np.ones(len(e), bool))):
        v = e[m]
        if not len(v):
            continue
        out[name] = {"decodes": int(len(v)),
                     "snr_db": {"mean": float(v[:, 1].mean()), "rms": float(np.sqrt((v[:, 1] ** 2).mean())), "worst": float(np.abs(v[:, 1]).max())},
                     "f_hz": {"mean": float(v[:, 2].mean()), "rms": float(np.sqrt((v[:, 2] ** 2).mean())), "worst": float(np.abs(v[:, 2]).max())},
                     "t_ms": {"mean": float(v[:, 3].mean()), "std": float(v[:, 3].std()), "worst": float(np.abs(v[:, 3]).max())}}
    return out


def measure_reports_twin(indices=range(0, 16)):
    made, missing = report_recipe_frames(indices)
    rows, default, edge = [], [], 0
    for i, x, truth in made:
        by_word, seen = {t["word"]: t for t in truth}, set()
        for r in ft4.decode_twin(x):
            t = by_word.get(r["word"])
            if t is None or r["word"] in seen:
                continue
            seen.add(r["word"])
            p = ft4.report(x, ft4.sig_from_record(r["f0"], r["h0"], r["tt"], r["ft"], r["word"]))
            edge += bool(p["flags"] & (ft4.RP_EDGE_T | ft4.RP_EDGE_F))
            rows.append((t["snr"], p["snr_db"] - t["snr"], p["f_hz"] - t["f0"], 1e3 * (p["t_sec"] - t["t0"])))
            default.append((t["snr"], r["snr"] - t["snr"], ft4.BIN_HZ * r["f0"] + ft4.DF_HZ * r["ft"] - t["f0"],
                            1e3 * ((ft4.HOP * r["h0"] + ft4.DT_STEP * r["tt"]) / ft4.FS - t["t0"])))
        print(f"reports twin frame {i}: {len(rows)} decodes so far", flush=True)
    return {"frames": [m[0] for m in made], "no_frame_at": missing, "planted": 8 * len(made), "on_a_border": edge,
            "report": report_stats(rows), "default_fields": report_stats(default)}


def measure_reports(B=256, warmup=2, steps=5, pairs=6):
    import torch
    from pyft8_amd import _lib
    from pyft8_amd.receiver import Receiver
    out = {}
    # ---- accuracy: frames 16 .. 79 through the receiver
    made, missing = report_recipe_frames(range(16, 80))
    audio = np.stack([m[1] for m in made])
    rx = Receiver("", None, max_frames=len(made), ft4_reports=True)
    res = rx.decode_frames_ft4(audio)
    rx.close()
    rows, default, edge, invalid = [], [], 0, 0
    for (i, _, truth), dicts in zip(made, res):
        by_text = {t["msg"]: t for t in truth}
        for d in dicts:
            t = by_text.get(" ".join(x for x in d["msg_tuple"] if x))
            if t is None:
                continue
            if d["report"] is None:
                invalid += 1
                continue
            rows.append((t["snr"], d["report"]["snr"] - t["snr"], d["report"]["fHz"] - t["f0"], 1e3 * (d["report"]["tsec"] - t["t0"])))
            default.append((t["snr"], int(d["their_snr"]) - t["snr"], d["fHz"] - t["f0"], 1e3 * (d["tsec"] - t["t0"])))
    out["accuracy_gpu"] = {"frames": [m[0] for m in made], "no_frame_at": missing, "planted": 8 * len(made), "invalid": invalid,
                           "report": report_stats(rows), "default_fields": report_stats(default)}
    print("reports accuracy", out["accuracy_gpu"]["report"], flush=True)
    # ---- the report stage at B = 256 with 20 signals per frame: its kernels by HIP events, the whole synchronous call by the clock
    a = np.stack([throughput_frame(k) for k in range(B)])
    h = _lib.Handle(max_frames=B)
    rec, cnt = h.ft4_decode(a)[:2]
    sigs = _lib.ft4_subtraction_list(rec, cnt)
    ptr = h.ft4_staging_ptr()
    for _ in range(warmup):
        h.ft4_report(ptr, sigs)
    t = []
    for _ in range(steps):
        t0 = time.perf_counter(); h.ft4_report(ptr, sigs); t.append(round(1e3 * (time.perf_counter() - t0), 3))
    h.set_profiling(True)
    stage = []
    for _ in range(steps):
        h.ft4_report(ptr, sigs); h.sync()
        stage.append({k: round(float(v), 4) for k, v in h.stage_times().items()})
    h.set_profiling(False)
    out["stage"] = {"B": B, "signals": int(sigs[1].sum()), "longest_list": int(sigs[1].max()), "call_ms": t, "kernel_ms": stage,
                    "workspace_bytes": h.ft4_report_info()["workspace_bytes"]}
    h.close()
    print("reports stage", out["stage"], flush=True)
    # ---- decode_frames_ft4 with the setting off and on, paired and alternating
    rxs = {"off": Receiver("", None, max_frames=B), "on": Receiver("", None, max_frames=B, ft4_reports=True)}
    for r in rxs.values():
        r.decode_frames_ft4(a)
    tt = {"off": [], "on": []}
    for _ in range(pairs):
        for name in ("off", "on"):
            t0 = time.perf_counter(); rxs[name].decode_frames_ft4(a); tt[name].append(round(1e3 * (time.perf_counter() - t0), 3))
    for r in rxs.values():
        r.close()
    out["receiver"] = {"B": B, "signals_per_frame": 20, "decode_frames_ft4_ms": tt,
                       "frames_per_s": {k: B / (1e-3 * float(np.median(v))) for k, v in tt.items()}}
    print("reports receiver", out["receiver"], flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ft4_measure.json"))
    ap.add_argument("--prob", action="store_true"); ap.add_argument("--noise", action="store_true"); ap.add_argument("--throughput", action="store_true")
    ap.add_argument("--twin", type=int, default=0); ap.add_argument("--passes", action="store_true")
    ap.add_argument("--noise-frames", type=int, default=2048); ap.add_argument("--coherent", action="store_true")
    ap.add_argument("--weak", action="store_true"); ap.add_argument("--coh-osd", action="store_true")
    ap.add_argument("--reports", action="store_true"); ap.add_argument("--reports-twin", action="store_true")
    args = ap.parse_args()
    if (args.reports or args.reports_twin) and args.out == ap.get_default("out"):
        args.out = os.path.join(ROOT, "profiles", "ft4_report_measure.json")
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if args.twin:
        res["twin_probability"] = measure_twin(args.twin)
    if args.prob or args.noise or args.throughput or args.coherent or args.weak or args.coh_osd:
        import torch  # noqa: F401 -- before libft8rx.so loads (_lib.lib)
        from pyft8_amd import _lib
        h = _lib.Handle(max_frames=256)
        if args.throughput:
            res["throughput"] = measure_throughput(h)
        if args.prob:
            res["probability"] = measure_prob(h)
        if args.noise:
            res["noise"] = measure_noise(h, args.noise_frames)
        if args.coherent:
            res["coherent"] = measure_coherent(h, args.noise_frames)
        if args.weak:
            res["weak"] = measure_weak(h, args.noise_frames)
        if args.coh_osd:
            res["coh_osd"] = measure_coh_osd(h, args.noise_frames)
        h.close()
    if args.passes:
        import torch  # noqa: F401,F811 -- before libft8rx.so loads (_lib.lib)
        res["passes"] = measure_passes()
    if args.reports_twin:
        res["accuracy_twin"] = measure_reports_twin()
    if args.reports:
        import torch  # noqa: F401,F811 -- before libft8rx.so loads (_lib.lib)
        res.update(measure_reports())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)
