"""Recall decoding of stations heard 30 s earlier (ipass 8, ft8rx_set_recall) on the GPU: the ladder is untouched, the scoring kernel
matches its numpy twin, the step decodes continuations below the sync floor and nothing else, it skips stations the ladder heard,
and the live receiver feeds it by itself."""
import threading
import time as _t

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

from conftest import ROOT, load_golden
from pyft8_amd import _lib, synth
from pyft8_amd import recall as R
from pyft8_amd.receiver import Receiver, decode_frames, frames_from_wav

pytestmark = pytest.mark.gpu
SENS_SNR = -20.0                    # the default decodes ~2 % of these continuations, recall most (profiles/recall_measure.json)
SENS_MARGIN = 40                    # over 32 frame pairs
PATTERNS = [(("CQ", "W9XYZ", "FN42"), ("CQ", "W9XYZ", "FN42")),
            (("K1ABC", "W8AAA", "-12"), ("K1ABC", "W8AAA", "RRR")),
            (("K2ABC", "W7BBB", "R-07"), ("K2ABC", "W7BBB", "RR73")),
            (("K3ABC", "W6CCC", "R-09"), ("K3ABC", "W6CCC", "73")),
            (("K4ABC", "W5DDD", "EM12"), ("K4ABC", "W5DDD", "-15")),
            (("K5ABC", "W4EEE", "-03"), ("K5ABC", "W4EEE", "R-11"))]


def _pairs(n, snr, seed0):
    rng = np.random.default_rng(seed0)
    a, b, truth = [], [], []
    for i in range(n):
        sa, sb, tr = [], [], []
        for k, (ta, tb) in enumerate(PATTERNS):
            f0 = 300.0 + 2400.0 * (k + 0.5) / len(PATTERNS) + rng.uniform(-20, 20)
            t0 = 0.5 + rng.uniform(-0.3, 0.8)
            sa.append((synth.pack77(*ta), f0, t0, 0.0))
            sb.append((synth.pack77(*tb), f0, t0, snr))
            tr.append((" ".join(tb), f0))
        a.append(synth.frame_with_signals(seed0 + 2 * i, sa))
        b.append(synth.frame_with_signals(seed0 + 2 * i + 1, sb))
        truth.append(tr)
    return np.stack(a), np.stack(b), truth


def _hits(dicts, truth):
    hit, wrong = 0, 0
    for f, ms in enumerate(dicts):
        for m in ms:
            t = " ".join(m["msg_tuple"])
            if any(t == x and abs(m["fHz"] - f0) < 10 for x, f0 in truth[f]):
                hit += 1
            elif m.get("recall"):
                wrong += 1
    return hit, wrong


@pytest.fixture(scope="module")
def corpus():
    names = ["test_08", "test_09", "synth_000000", "synth_100000", "synth_200000"]
    audio = [load_golden(n)[0] for n in names]
    for wav in ("test_08.wav", "test_09.wav"):
        audio += list(frames_from_wav(f"{ROOT}/tests/golden/{wav}"))
    return np.stack(audio)


@pytest.fixture(scope="module")
def sens():
    fa, fb, truth = _pairs(32, SENS_SNR, 7000)
    prev = decode_frames(fa)
    return fa, fb, truth, prev


def _ev_sorted(ev, n):
    return np.sort(ev[:n], order=["cand", "ipass", "slot", "seq"]).tobytes()


def test_ladder_unchanged(corpus):
    """Entries set (those of the frames themselves, and random ones): the ladder's records, counts, events and messages are
    byte-identical to recall off; set with no entries, everything is."""
    B = len(corpus)
    h = _lib.Handle(max_frames=B)
    try:
        ra, ca, ea, eca = h.decode_batch(corpus)
        ma, na = _lib.package_batch(ra, ca, ea, eca)
        own = [R.entries_from_rows(ma[f], na[f], h.cfg) for f in range(B)]
        rng = np.random.default_rng(1)
        rnd = [np.array([R._entry(synth.pack77(*synth.random_message(rng)), int(rng.integers(40, 900)), int(rng.integers(-30, 80)))
                         for _ in range(20)], _lib.RECALL_ENTRY_DTYPE) for _ in range(B)]
        for ents in (own, rnd):
            h.set_recall(ents)
            rb, cb, eb, ecb = h.decode_batch(corpus)
            rr, rc = h.fetch_recall(B)
            assert np.array_equal(ca, cb) and np.array_equal(eca, ecb)
            for f in range(B):
                assert ra[f, :ca[f]].tobytes() == rb[f, :cb[f]].tobytes()
                ne = min(int(eca[f]), _lib.EVENT_CAP)
                assert _ev_sorted(ea[f], ne) == _ev_sorted(eb[f], ne)
            mb, nb = _lib.package_batch(rb, cb, eb, ecb)
            assert ma.tobytes() == mb.tobytes() and na.tobytes() == nb.tobytes()
            assert rc.tolist() == [len(e) for e in ents]
        # own entries: every station was heard by the ladder -> all skipped
        h.set_recall(own)
        h.decode_batch(corpus)
        rr, rc = h.fetch_recall(B)
        assert (rr["ipass"] == 0).all()
        # no entries: byte-identical in everything, and nothing appended
        h.set_recall([[] for _ in range(B)])
        rb, cb, eb, ecb = h.decode_batch(corpus)
        rr, rc = h.fetch_recall(B)
        assert not rc.any() and rb.tobytes() == ra.tobytes() and np.array_equal(ecb, eca)
        mr, nr = _lib.package_batch_recall(rb, cb, eb, ecb, rr, rc)
        assert np.array_equal(nr, na) and all(mr[f, :nr[f]].tobytes() == ma[f, :na[f]].tobytes() for f in range(B))
        # the setting is consumed by one batch
        rb, cb, eb, ecb = h.decode_batch(corpus)
        assert not h.fetch_recall(B)[1].any()
    finally:
        h.close()
    d0 = decode_frames(corpus)
    assert all("recall" not in m for f in d0 for m in f)


def test_probe_matches_twin(sens):
    """ft8rx_recall_probe on crafted grids and on real fine grids: words and hd equal the numpy twin exactly, D to 1e-5, and the
    choice and acceptance are identical."""
    fa, fb, truth, prev = sens
    rng = np.random.default_rng(2)
    grids, ents = [], []
    for k in range(40):                                       # crafted: a hypothesis' tones, or another word's, in noise
        ta, tb = PATTERNS[k % len(PATTERNS)]
        w_ent = synth.pack77(*ta)
        sent = synth.pack77(*tb) if k % 3 else synth.pack77(*synth.random_message(rng))
        g = np.abs(rng.normal(0, 0.3 + 0.02 * k, (79, 8))).astype(np.float32) + 0.01
        for s, tone in enumerate(synth.tones79(sent)):
            g[s, tone] += 1.0
        grids.append(g)
        ents.append(R._entry(w_ent, 300, 10))
    h = _lib.Handle(max_frames=len(fb))
    try:
        spec = h.cycle_spectrum(fb[:8])
        for f in range(8):                                    # real: the forced fine sync's grids at the entries of cycle n
            for e in R.entries_from_dicts(prev[f], h.cfg):
                out = h.fine(spec, [f], [int(e["f0_idx"])], [int(e["h0_idx"])], want_sgrid=True)
                grids.append(out["sgrid"][0])
                ents.append(e)
        recs = h.recall_probe(np.stack(grids), np.array(ents, _lib.RECALL_ENTRY_DTYPE))
    finally:
        h.close()
    n_acc = 0
    for g, e, r in zip(grids, ents, recs):
        w = (int(e["msg_hi"]) << 64) | int(e["msg_lo"])
        t = R.score(g, w)
        assert r["ipass"] == 8 and r["method"] == _lib.M_RECALL
        assert (int(r["msg_hi"]) << 64) | int(r["msg_lo"]) == t["word"]
        assert (int(r["osd_hd"]), int(r["pad2"]), int(r["n_its"]), int(r["ap"])) == (t["hd"], t["hd2"], t["index"], t["cls"])
        assert float(r["score"]) == pytest.approx(t["D"], rel=1e-5)
        if t["D2"] >= 0:
            assert float(r["grid_sd"]) == pytest.approx(t["D2"], rel=1e-5)
        assert (int(r["status"]) == _lib.ST_DECODED) == t["accept"]
        n_acc += t["accept"]
    assert 0 < n_acc < len(recs)


def test_sensitivity(sens):
    """Continuations at SENS_SNR of stations heard at 0 dB 30 s earlier: recall decodes SENS_MARGIN more of them than the default
    over 32 frame pairs, and no wrong message."""
    fa, fb, truth, prev = sens
    d0 = decode_frames(fb)
    d1 = decode_frames(fb, recall=prev)
    h0, w0 = _hits(d0, truth)
    h1, w1 = _hits(d1, truth)
    print("default", h0, "recall", h1, "wrong", w1)
    assert h1 >= h0 + SENS_MARGIN and w1 == 0
    assert all(("recall" in m) for f in d1 for m in f)
    assert any(m["recall"] and m["decode_notes"].startswith("fine_RECALL_") for f in d1 for m in f)
    for f in range(len(fb)):                                  # the default's messages come first, unchanged
        texts0 = [" ".join(m["msg_tuple"]) for m in d0[f]]
        texts1 = [" ".join(m["msg_tuple"]) for m in d1[f]]
        assert texts1[:len(texts0)] == texts0 and len(set(texts1)) == len(texts1)


def test_no_false_decodes():
    """Absent-station history on config-1 frames (30 entries) and noise frames (64 entries): no recall decode at the defaults."""
    B = 128
    h = _lib.Handle(max_frames=B)
    d = torch.empty((B, synth.NFRAME), dtype=torch.int16, device="cuda")
    rng = np.random.default_rng(9)
    n_dec = n_test = 0
    try:
        for start, nsig, ne in ((0, 50, 30), (20_000_000, 0, 64)):
            h.synth_frames(d.data_ptr(), start, B, n_signals=nsig)
            torch.cuda.synchronize()
            h.set_recall([[R._entry(synth.pack77(*synth.random_message(rng)), int(rng.integers(h.cfg.f0_lo, h.cfg.f0_hi)),
                                    int(rng.integers(h.cfg.h0_lo, h.cfg.h0_hi))) for _ in range(ne)] for _ in range(B)])
            h.enqueue(d.data_ptr(), B)
            h.fetch(B)
            rr, rc = h.fetch_recall(B)
            n_test += int((rr["ipass"] == 8).sum())
            n_dec += int(((rr["ipass"] == 8) & (rr["status"] == _lib.ST_DECODED)).sum())
    finally:
        h.close()
    assert n_test > 0.9 * B * 64 and n_dec == 0


def test_skip_rule():
    """An entry whose station the ladder decodes (at 0 dB) gets no ipass-8 record; the same entry where only a weak signal is gets one."""
    w = synth.pack77("K1ABC", "W9XYZ", "RR73")
    strong = synth.frame_with_signals(1, [(w, 1000.0, 0.5, 0.0)])
    h = _lib.Handle(max_frames=1)
    try:
        rec, cnt, ev, evc = h.decode_batch(strong)
        dec = rec[0][:cnt[0]][rec[0][:cnt[0]]["status"] == _lib.ST_DECODED]
        assert len(dec) >= 1
        r = dec[0]
        e = R._entry(synth.pack77("K1ABC", "W9XYZ", "-10"), int(r["f0_idx"]) + 1, int(r["h0_idx"]) - 3)
        h.set_recall([[e]])
        h.decode_batch(strong)
        rr, rc = h.fetch_recall(1)
        assert rc[0] == 1 and rr[0, 0]["ipass"] == 0
        h.set_recall([[e]])
        h.decode_batch(synth.frame_with_signals(2, [(w, 1000.0, 0.5, -30.0)]))
        rr, rc = h.fetch_recall(1)
        assert rr[0, 0]["ipass"] == 8
    finally:
        h.close()


def test_with_ap_calls(sens):
    """my_call set as well: the union of both steps' messages, no text twice."""
    fa, fb, truth, prev = sens
    dr = decode_frames(fb, recall=prev)
    da = decode_frames(fb, my_call="K2ABC", dx_call="W7BBB")
    db = decode_frames(fb, recall=prev, my_call="K2ABC", dx_call="W7BBB")
    for f in range(len(fb)):
        tb = [" ".join(m["msg_tuple"]) for m in db[f]]
        assert len(tb) == len(set(tb))
        assert set(tb) == {" ".join(m["msg_tuple"]) for m in dr[f]} | {" ".join(m["msg_tuple"]) for m in da[f]}


def test_refusals(corpus):
    with pytest.raises(_lib.Ft8rxError, match="msg_types"):
        Receiver("", None, recall=True, msg_types="all")
    rx = Receiver("", None, recall=True, max_frames=2)
    with pytest.raises(_lib.Ft8rxError, match="passes"):
        rx.decode_frames(corpus[:2], passes=2)
    with pytest.raises(_lib.Ft8rxError, match="decode_frames_arrays"):
        rx.decode_frames_arrays(corpus[:2])
    rx.close()
    h = _lib.Handle(max_frames=2)
    try:
        h.set_recall([[R._entry(synth.pack77("K1ABC", "W9XYZ", "-10"), 300, 10)], []])
        with pytest.raises(_lib.Ft8rxError, match="ft8rx_set_recall"):
            h.decode_messages(corpus[:2])
        with pytest.raises(_lib.Ft8rxError, match="outside the search range"):
            h.set_recall([[R._entry(synth.pack77("K1ABC", "W9XYZ", "-10"), 5000, 10)], []])
        with pytest.raises(_lib.Ft8rxError, match="at most"):
            h.set_recall([[R._entry(synth.pack77("K1ABC", "W9XYZ", "-10"), 300, 10)] * 65, []])
        h.set_recall(None)
    finally:
        h.close()


def _live(recall, cycles, snr_cont):
    """Receiver fed cycle 1 (the stations at 0 dB), cycle 2 (noise), cycle 3 (their continuations at snr_cont) through audio_source
    under a virtual clock -> messages of cycle 3 (start 30 s)."""
    sa, sb = [], []
    rng = np.random.default_rng(11)
    for k, (ta, tb) in enumerate(PATTERNS):
        f0, t0 = 300.0 + 400.0 * k + rng.uniform(-20, 20), 0.5 + rng.uniform(-0.2, 0.6)
        sa.append((synth.pack77(*ta), f0, t0, 0.0))
        sb.append((synth.pack77(*tb), f0, t0, snr_cont))
    stream = np.concatenate([synth.frame_with_signals(301, sa), synth.frame_with_signals(302, []), synth.frame_with_signals(303, sb),
                             np.zeros(180000, np.int16)])
    vt = [0.0]
    lock = threading.Lock()
    got = []

    def hops():
        for k in range(cycles * 375):
            with lock:
                vt[0] = (k + 1) * 0.04 + 0.12
            yield stream[480 * k:480 * k + 480]
            _t.sleep(0.0005)
        _t.sleep(0.5)

    rx = Receiver("any", got.append, time_source=lambda: vt[0], sleep=lambda dt: _t.sleep(0.002), audio_source=hops(),
                  early_decode_hop=None, recall=recall)
    try:
        deadline = _t.time() + 180
        while not getattr(rx.audio_in, "source_exhausted", False) and _t.time() < deadline:
            _t.sleep(0.05)
        _t.sleep(0.5)
    finally:
        rx.stop()
    assert rx.thread_error is None
    conts = {" ".join(tb) for _, tb in PATTERNS}
    return [m for m in got if m["cyclestart_string"].endswith("000030") and " ".join(m["msg_tuple"]) in conts], got


def test_live_receiver():
    """Receiver(recall=True) delivers weak continuations in cycle 3 from what it heard in cycle 1; recall=False does not."""
    on, all_on = _live(True, 4, -21.0)
    off, _ = _live(False, 4, -21.0)
    print("recall", len(on), "default", len(off))
    assert len(on) > len(off) and all(m["recall"] for m in on)
    assert all("recall" in m for m in all_on)
