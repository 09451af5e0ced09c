"""Measurements behind the recall step's default gates (ipass 8, ft8rx_set_recall).

    python tools/recall_measure.py --out profiles/recall_measure.json [--quick]

  noise     device-synthesised noise-only frames, 64 random entries per frame, gates open: histograms of hd_best and of the gap
            (runner-up hd - best hd), and the decodes the default gates would accept
  absent    the config-1 workload (device generator, 256 frames), 30 entries per frame of random calls at random positions that nobody
            transmits: the same histograms, the nearest false hd / gap
  snr       -24 .. -18 dB, frame pairs: cycle n carries `A B X` at 0 dB, cycle n + 2 the continuation at the same (f0, t0) at the test SNR
            (one station per class: repeat, RRR, RR73, 73, report, R-report); decode_frames with and without the messages of cycle n
  true      the hd_best / gap of every TRUE continuation the open gate finds in the snr runs (what the gates must keep)
  cost      decode_frames-equivalent (set_recall + decode_batch + fetch_recall) on 256 config-1 frames with 30 entries each vs without,
            median of 10 alternating runs
Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyft8_amd import _lib, synth  # noqa: E402
from pyft8_amd import recall as R  # noqa: E402
from pyft8_amd.receiver import decode_frames  # noqa: E402

# (entry text of cycle n, continuation of cycle n + 2, class)
PATTERNS = [(("CQ", "W9XYZ", "FN42"), ("CQ", "W9XYZ", "FN42"), "repeat"),
            (("K1ABC", "W8AAA", "-12"), ("K1ABC", "W8AAA", "RRR"), "RRR"),
            (("K2ABC", "W7BBB", "R-07"), ("K2ABC", "W7BBB", "RR73"), "RR73"),
            (("K3ABC", "W6CCC", "R-09"), ("K3ABC", "W6CCC", "73"), "73"),
            (("K4ABC", "W5DDD", "EM12"), ("K4ABC", "W5DDD", "-15"), "report"),
            (("K5ABC", "W4EEE", "-03"), ("K5ABC", "W4EEE", "R-11"), "R-report")]


def random_entries(rng, n, cfg):
    out = np.zeros(n, _lib.RECALL_ENTRY_DTYPE)
    for i in range(n):
        w = synth.pack77(*synth.random_message(rng))
        out[i] = R._entry(w, int(rng.integers(cfg.f0_lo, cfg.f0_hi)), int(rng.integers(cfg.h0_lo, cfg.h0_hi)))
    return out


def hist(v, lo=0, hi=175):
    h = np.bincount(np.clip(np.asarray(v, np.int64), lo, hi - 1) - lo, minlength=hi - lo)
    return {str(i + lo): int(c) for i, c in enumerate(h) if c}


def tested(rec):
    return rec[(rec["ipass"] == 8)]


def gate_stats(rs, max_hd, min_gap):
    one = rs["grid_sd"] < 0                   # a single hypothesis (CQ / QRZ / DE entries): no runner-up, hd2 = 174
    return dict(_gate_stats(rs, max_hd, min_gap), single_hypothesis=_gate_stats(rs[one], max_hd, min_gap),
                call_entries=_gate_stats(rs[~one], max_hd, min_gap))


def _gate_stats(rs, max_hd, min_gap):
    hd = rs["osd_hd"].astype(int)
    gap = rs["pad2"].astype(int) - hd
    acc = (hd <= max_hd) & (gap >= min_gap)
    return dict(tested=int(len(rs)), hd_best_hist=hist(hd), gap_hist=hist(gap, -174, 175), min_hd=int(hd.min()) if len(hd) else None,
                max_gap=int(gap.max()) if len(gap) else None, accepted_at_defaults=int(acc.sum()),
                nearest=sorted([(int(a), int(b)) for a, b in zip(hd, gap)], key=lambda t: (t[0] - t[1]))[:5])


def run_device(h, d, start, B, entries, n_signals):
    h.synth_frames(d.data_ptr(), start, B, n_signals=n_signals)
    torch.cuda.synchronize()
    h.set_recall(entries)
    h.enqueue(d.data_ptr(), B)
    rec, cnt, ev, evc = h.fetch(B)
    return h.fetch_recall(B)[0].reshape(-1)


def measure_noise(n_frames, B, seed):
    rng = np.random.default_rng(seed)
    h = _lib.Handle(max_frames=B)
    h.set_recall_gates(174, 0)
    d = torch.empty((B, synth.NFRAME), dtype=torch.int16, device="cuda")
    rs = []
    for k in range(n_frames // B):
        ents = [random_entries(rng, 64, h.cfg) for _ in range(B)]
        rs.append(tested(run_device(h, d, 30_000_000 + k * B, B, ents, 0)))
    h.close()
    return np.concatenate(rs)


def measure_absent(B, seed):
    rng = np.random.default_rng(seed)
    h = _lib.Handle(max_frames=B)
    h.set_recall_gates(174, 0)
    d = torch.empty((B, synth.NFRAME), dtype=torch.int16, device="cuda")
    ents = [random_entries(rng, 30, h.cfg) for _ in range(B)]
    r = tested(run_device(h, d, 0, B, ents, 50))
    h.close()
    return r


def pair_frames(snr, n_pairs, seed0):
    rng = np.random.default_rng(seed0)
    a, b, truth = [], [], []
    for i in range(n_pairs):
        sig_a, sig_b, tr = [], [], []
        for k, (ta, tb, cls) in enumerate(PATTERNS):
            f0 = 300.0 + 2400.0 * (k + 0.5) / len(PATTERNS) + rng.uniform(-20, 20)
            t0 = 0.5 + rng.uniform(-0.3, 0.8)
            sig_a.append((synth.pack77(*ta), f0, t0, 0.0))
            sig_b.append((synth.pack77(*tb), f0, t0, snr))
            tr.append((" ".join(tb), f0, cls))
        a.append(synth.frame_with_signals(seed0 + 2 * i, sig_a))
        b.append(synth.frame_with_signals(seed0 + 2 * i + 1, sig_b))
        truth.append(tr)
    return np.stack(a), np.stack(b), truth


def score_pairs(dicts, truth):
    hit, wrong = {c: 0 for _, _, c in PATTERNS}, 0
    for f, ms in enumerate(dicts):
        for m in ms:
            t = " ".join(m["msg_tuple"])
            match = [c for (txt, f0, c) in truth[f] if txt == t and abs(m["fHz"] - f0) < 10]
            if match:
                hit[match[0]] += 1
            elif m.get("recall"):
                wrong += 1
    return hit, wrong


def measure_snr(snrs, n_pairs, open_gate_records):
    out = []
    for snr in snrs:
        fa, fb, truth = pair_frames(snr, n_pairs, 5000 + int((snr + 30) * 10) * 1000)
        prev = decode_frames(fa)
        d0 = decode_frames(fb)
        d1 = decode_frames(fb, recall=prev)
        h0, w0 = score_pairs(d0, truth)
        h1, w1 = score_pairs(d1, truth)
        n_prev = sum(len(p) for p in prev)
        # open gate: the hd / gap of the true continuations (and the rest)
        h = _lib.Handle(max_frames=len(fb))
        h.set_recall_gates(174, 0)
        h.set_recall([R.entries_from_dicts(p, h.cfg) for p in prev])
        h.decode_batch(fb)
        rr, rc = h.fetch_recall(len(fb))
        h.close()
        true_words = {synth.pack77(*tb) for _, tb, _ in PATTERNS}
        for r in tested(rr.reshape(-1)):
            w = (int(r["msg_hi"]) << 64) | int(r["msg_lo"])
            open_gate_records.append((int(r["osd_hd"]), int(r["pad2"]) - int(r["osd_hd"]), w in true_words, float(snr), bool(r["grid_sd"] < 0)))
        out.append(dict(snr=snr, pairs=n_pairs, entries_cycle_n=n_prev, default=h0, recall=h1, default_total=sum(h0.values()),
                        recall_total=sum(h1.values()), wrong_default=w0, wrong_recall=w1))
        print(out[-1], flush=True)
    return out


def measure_cost(B, seed, reps):
    rng = np.random.default_rng(seed)
    h = _lib.Handle(max_frames=B)
    d = torch.empty((B, synth.NFRAME), dtype=torch.int16, device="cuda")
    h.synth_frames(d.data_ptr(), 0, B)
    torch.cuda.synchronize()
    audio = d.cpu().numpy()
    ents = [random_entries(rng, 30, h.cfg) for _ in range(B)]
    t_off, t_on = [], []
    h.decode_batch(audio)
    for _ in range(reps):
        t = time.perf_counter(); h.decode_batch(audio); t_off.append(time.perf_counter() - t)
        t = time.perf_counter(); h.set_recall(ents); h.decode_batch(audio); h.fetch_recall(B); t_on.append(time.perf_counter() - t)
    h.close()
    return dict(frames=B, entries_per_frame=30, reps=reps, ms_without=float(np.median(t_off) * 1e3), ms_with=float(np.median(t_on) * 1e3),
                all_without=[round(x * 1e3, 3) for x in t_off], all_with=[round(x * 1e3, 3) for x in t_on])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/recall_measure.json")
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    res = {"defaults": {"max_hd": _lib.RECALL_MAX_HD_DEFAULT, "min_gap": _lib.RECALL_MIN_GAP_DEFAULT}}
    D, G = _lib.RECALL_MAX_HD_DEFAULT, _lib.RECALL_MIN_GAP_DEFAULT
    nz = measure_noise(256 if a.quick else 2048, 256, 1)
    res["noise"] = dict(frames=256 if a.quick else 2048, entries_per_frame=64, **gate_stats(nz, D, G))
    print("noise", res["noise"]["tested"], res["noise"]["min_hd"], res["noise"]["max_gap"], res["noise"]["accepted_at_defaults"], flush=True)
    ab = measure_absent(256, 2)
    res["absent"] = dict(frames=256, entries_per_frame=30, **gate_stats(ab, D, G))
    print("absent", res["absent"]["tested"], res["absent"]["min_hd"], res["absent"]["max_gap"], res["absent"]["accepted_at_defaults"], flush=True)
    og = []
    res["snr"] = measure_snr([-24.0, -23.0, -22.0, -21.0, -20.0, -19.0, -18.0], 16 if a.quick else 64, og)
    tru = [t for t in og if t[2]]
    fal = [t for t in og if not t[2]]
    res["true_open_gate"] = dict(n=len(tru), hd_hist=hist([t[0] for t in tru]), gap_hist=hist([t[1] for t in tru], -174, 175),
                                 kept_at_defaults=int(sum(1 for t in tru if t[0] <= D and t[1] >= G)),
                                 all=[t[:2] + (t[3], t[4]) for t in tru])
    res["false_open_gate_all"] = [t[:2] + (t[3], t[4]) for t in fal]
    res["false_open_gate_snr_runs"] = dict(n=len(fal), accepted_at_defaults=int(sum(1 for t in fal if t[0] <= D and t[1] >= G)),
                                           min_hd=min((t[0] for t in fal), default=None), max_gap=max((t[1] for t in fal), default=None))
    res["cost"] = measure_cost(256, 3, 10)
    print("cost", res["cost"]["ms_without"], res["cost"]["ms_with"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
