"""Measured signal reports (ft8rx_set_reports) on the GPU: the default is untouched, the setting changes no
record, k_report agrees with the float64 twin (pyft8_amd/report.py) on the GPU's own cycle spectrum and with the probe byte for
byte, the reports meet the accuracy bounds on synthetic truth, the allowed combinations carry them, the refused ones say why, and
the live path delivers them."""
import threading
import time as _t

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

from conftest import ROOT, load_golden
from pyft8_amd import _lib, synth
from pyft8_amd import messages as M
from pyft8_amd import report as R
from pyft8_amd.receiver import Receiver, config_from_kwargs, decode_frames, frames_from_wav
from test_report import check_bounds, recipe_frame

pytestmark = pytest.mark.gpu
MY, DX = "K1ABC", "W9XYZ"


@pytest.fixture(scope="module")
def corpus():
    names = ["test_08", "test_09", "synth_000000", "synth_100000", "synth_200000"]
    audio = [load_golden(n)[0] for n in names]
    for wav in ("test_08.wav", "test_09.wav"):
        audio += list(frames_from_wav(f"{ROOT}/tests/golden/{wav}"))
    return np.stack(audio)


@pytest.fixture(scope="module")
def recipe():
    """64 frames of the CPU test's recipe, indices continuing after its 16 -> (audio [64, 180000], truth per frame)."""
    frames = [recipe_frame(i) for i in range(16, 80)]
    return np.stack([f[0] for f in frames]), [f[1] for f in frames]


def _run(audio, mode="on", **kw):
    """One batch on a fresh handle.  mode: "never" (the setting never made), "cleared" (made, then cleared), "on".
    -> dict(rec, cnt, ev, evc, rp, spec): rp / spec (the GPU's own cycle spectrum) only with the setting on."""
    cfg = config_from_kwargs(**kw)
    h = _lib.Handle(cfg, max_frames=len(audio))
    try:
        if mode != "never":
            h.set_reports(True)
        if mode == "cleared":
            h.set_reports(False)
        rec, cnt, ev, evc = h.decode_batch(audio)
        out = dict(rec=rec, cnt=cnt, ev=ev, evc=evc, rp=h.fetch_reports(len(audio)))
        if mode == "on":
            out["spec"] = h.cycle_spectrum(audio)
        return out
    finally:
        h.close()


def _ev_sorted(ev, n):
    return np.sort(ev[:n], order=["cand", "ipass", "slot", "seq"]).tobytes()


def _same_results(a, b):
    assert np.array_equal(a["cnt"], b["cnt"]) and np.array_equal(a["evc"], b["evc"])
    for f in range(len(a["cnt"])):
        assert a["rec"][f, :a["cnt"][f]].tobytes() == b["rec"][f, :b["cnt"][f]].tobytes(), f
        ne = min(int(a["evc"][f]), _lib.EVENT_CAP)
        assert _ev_sorted(a["ev"][f], ne) == _ev_sorted(b["ev"][f], ne), f


@pytest.fixture(scope="module")
def sets(corpus, recipe):
    """The three sets with the setting on, decoded once and left unchanged."""
    audio = {"corpus": corpus, "synth": synth.make_batch(0, 16), "recipe": recipe[0]}
    return {k: (a, _run(a)) for k, a in audio.items()}


def _strip(L):
    return [[{k: v for k, v in m.items() if k != "decode_completed"} for m in f] for f in L]


def test_default_unchanged(corpus):
    """The setting never made, or made and cleared again: records, events, packaged messages and dicts are byte-identical, nothing
    carries a report."""
    a, b = _run(corpus, "never"), _run(corpus, "cleared")
    _same_results(a, b)
    ma, na = _lib.package_batch(a["rec"], a["cnt"], a["ev"], a["evc"])
    mb, nb = _lib.package_batch(b["rec"], b["cnt"], b["ev"], b["evc"])
    assert ma.tobytes() == mb.tobytes() and na.tobytes() == nb.tobytes() and na.sum() > 0
    assert not a["rp"].view(np.uint8).any() and not b["rp"].view(np.uint8).any()
    d0, d1 = decode_frames(corpus), decode_frames(corpus, reports=False)
    assert _strip(d0) == _strip(d1) and all("report" not in m for f in d0 for m in f)


def test_records_unchanged_with_reports(corpus, sets):
    """With the setting on the ladder's records, counts and events are those of the default; every DECODED slot has a report, no
    other slot has one; the reference's keys of the message dicts stay as they are."""
    for audio, on in (sets["corpus"], sets["synth"]):
        off = _run(audio, "never")
        _same_results(off, on)
        n = 0
        for f in range(len(audio)):
            dec = np.zeros(on["rec"].shape[1], bool)
            dec[:on["cnt"][f]] = on["rec"][f, :on["cnt"][f]]["status"] == _lib.ST_DECODED
            assert np.array_equal(on["rp"][f]["flags"] & _lib.RP_MEASURED != 0, dec), f
            assert not on["rp"][f][~dec].view(np.uint8).any()
            n += int(dec.sum())
        assert n > 50
    d0, d1 = decode_frames(corpus[:4]), decode_frames(corpus[:4], reports=True)
    assert _strip(d0) == [[{k: v for k, v in m.items() if k != "report"} for m in f] for f in _strip(d1)]
    assert all(m["report"] is None or set(m["report"]) == {"snr", "fHz", "tsec"} for f in d1 for m in f) and sum(map(len, d1)) > 0


def _decoded(res):
    """(frame, cand) of every DECODED record"""
    return [(f, i) for f in range(len(res["cnt"])) for i in range(int(res["cnt"][f])) if res["rec"][f, i]["status"] == _lib.ST_DECODED]


def _probe(audio, res, **kw):
    """The probe on the same spectra for every DECODED record of a batch -> reports in _decoded order."""
    who = _decoded(res)
    r = [res["rec"][f, i] for f, i in who]
    h = _lib.Handle(config_from_kwargs(**kw), max_frames=len(audio))
    try:
        return who, h.report_probe(res["spec"], [f for f, _ in who], [x["f0_idx"] for x in r], [x["h0_idx"] for x in r],
                                   [x["ttweak"] for x in r], [x["ftweak"] for x in r], [(int(x["msg_hi"]) << 64) | int(x["msg_lo"]) for x in r])
    finally:
        h.close()


def _probe_equals_batch(audio, res, **kw):
    who, pr = _probe(audio, res, **kw)
    assert len(who) > 0
    batch = np.array([res["rp"][f, i] for f, i in who], _lib.REPORT_DTYPE)
    assert pr.tobytes() == batch.tobytes()
    return who, batch


def test_matches_twin(sets):
    """Every DECODED record of the corpus, of synth.make_batch(0, 16) and of 64 recipe frames: the batch's report equals the twin on the
    GPU's own cycle spectrum within 0.01 Hz, 0.05 ms and 0.05 dB, and the probe returns the batch's bytes.  A decode whose two best
    score cells lie within 1e-5 relative in the twin may pick the other cell in float32 and is left out (at most 1 %)."""
    total = left_out = 0
    worst = np.zeros(3)
    for name, (audio, res) in sets.items():
        who, batch = _probe_equals_batch(audio, res)
        for (f, i), got in zip(who, batch):
            x = res["rec"][f, i]
            tw = R.measure(res["spec"][f], int(x["f0_idx"]), int(x["h0_idx"]), int(x["ttweak"]), int(x["ftweak"]), (int(x["msg_hi"]) << 64) | int(x["msg_lo"]))
            total += 1
            if tw is None:
                assert got["flags"] == _lib.RP_MEASURED | _lib.RP_INVALID and np.isnan([got["snr_db"], got["f_hz"], got["t_sec"]]).all()
                continue
            top = np.sort(tw["P"].ravel())[-2:]
            if top[1] - top[0] <= 1e-5 * top[1]:
                left_out += 1
                continue
            assert int(got["flags"]) == tw["flags"], (name, f, i)
            err = np.abs([got["f_hz"] - tw["f_hz"], got["t_sec"] - tw["t_sec"], got["snr_db"] - tw["snr_db"]])
            worst = np.maximum(worst, err)
            assert err[0] <= 0.01 and err[1] <= 0.05e-3 and err[2] <= 0.05, (name, f, i, err, dict(x=x, got=got, tw={k: v for k, v in tw.items() if k != "P"}))
    print(f"matches_twin: {total} decodes, {left_out} left out as ties; worst |f| {worst[0]:.2e} Hz, |t| {worst[1]:.2e} s, |snr| {worst[2]:.2e} dB")
    assert total > 800 and left_out <= total // 100


def test_accuracy_on_the_gpu(recipe):
    """The CPU test's bounds on the GPU's reports for 64 frames of the recipe; the default snr / fHz / tsec of the same dicts are those
    of a receiver without the setting."""
    audio, truth = recipe
    d_on, d_off = decode_frames(audio, reports=True), decode_frames(audio)
    assert _strip(d_off) == [[{k: v for k, v in m.items() if k != "report"} for m in f] for f in _strip(d_on)]
    tr, got, dflt = [], [], []
    for f, sig in enumerate(truth):
        by_text = {s[4]: s for s in sig}
        for m in d_on[f]:
            if m["msg_tuple"] not in by_text:
                continue
            _, f0, t0, snr, _ = by_text.pop(m["msg_tuple"])
            assert m["report"] is not None
            tr.append((snr, f0, t0))
            got.append((m["report"]["snr"], m["report"]["fHz"], m["report"]["tsec"]))
            dflt.append((int(m["their_snr"]), m["fHz"], m["tsec"]))
    e = np.array(dflt, float) - np.array(tr, float)
    print("default fields on the same messages: snr mean %.2f std %.2f worst %.2f, f mean %.3f std %.3f, t mean %.4f std %.4f"
          % (e[:, 0].mean(), e[:, 0].std(), np.abs(e[:, 0]).max(), e[:, 1].mean(), e[:, 1].std(), e[:, 2].mean(), e[:, 2].std()))
    check_bounds(tr, got, 640)


def _all_reported(audio, res, **kw):
    """Every DECODED record of a batch has a valid report, equal to the probe's."""
    who, batch = _probe_equals_batch(audio, res, **kw)
    assert (batch["flags"] & (_lib.RP_MEASURED | _lib.RP_INVALID) == _lib.RP_MEASURED).all() and np.isfinite(batch["snr_db"]).all()
    return who


def test_combinations_and_refusals():
    # message types: the word is re-encoded whatever its type
    free = synth.pack77_ext("TNX BOB 73 GL")
    audio = np.stack([synth.frame_with_signals(900 + i, [(free, 1000.0 + 50 * i, 0.6, 0.0), (synth.pack77("CQ", "G4XYZ", "IO91"), 1800.0, 0.3, -5.0)])
                      for i in range(2)])
    res = _run(audio, msg_types="all")
    _all_reported(audio, res, msg_types="all")
    d = decode_frames(audio, msg_types="all", reports=True)
    ft = [m for f in d for m in f if m["msg_tuple"][0] == "TNX BOB 73 GL"]
    # sent at 0 dB: three times the RMS bounds of the accuracy test (0.25 Hz, 1.5 dB) for a single value
    assert len(ft) == 2 and all(abs(m["report"]["fHz"] - (1000.0 + 50 * i)) < 0.75 and abs(m["report"]["snr"]) < 4.5 for i, m in enumerate(ft)), ft
    # a-priori calls: ipass 7 included
    words = [synth.pack77(MY, DX, "RR73"), synth.pack77(MY, DX, "73"), synth.pack77(MY, DX, "RRR"), synth.pack77(MY, DX, "-15"),
             synth.pack77("CQ", DX, "FN42"), synth.pack77(MY, "G4ABC", "-07")]
    audio = np.stack([synth.frame_from_words(40 + i, words, snr_range=(-19.0, -19.0)) for i in range(24)])      # where ipass 7 adds decodes
    res = _run(audio, my_call=MY, dx_call=DX)
    who = _all_reported(audio, res, my_call=MY, dx_call=DX)
    n7 = sum(int(res["rec"][f, i]["ipass"]) == 7 for f, i in who)
    print("ipass-7 records with a report:", n7, "of", len(who))
    assert n7 >= 1
    # weak mode: the window is centred on the record's own tweaks
    audio = np.stack([synth.frame_from_words(60 + i, words, snr_range=(-20.0, -18.0)) for i in range(4)])
    res = _run(audio, weak=True)
    _all_reported(audio, res, weak=True)
    # recall: its own ipass-8 messages carry None
    spots = [(("K1ABC", "W9XYZ"), 500.0, 0.4), (("G4ABC", "PA3XYZ"), 900.0, 0.7), (("JA1XYZ", "VE3ABC"), 1300.0, 0.5), (("N0CALL", "DL1ABC"), 1700.0, 0.9),
             (("W1AW", "K9AAA"), 2100.0, 0.6), (("EA5XYZ", "OH2ABC"), 2500.0, 0.8)]
    first = synth.frame_with_signals(950, [(synth.pack77(a, b, "-10"), f0, t0, 0.0) for (a, b), f0, t0 in spots])
    cont = synth.frame_with_signals(951, [(synth.pack77(a, b, "RR73"), f0, t0, -20.5) for (a, b), f0, t0 in spots] +
                                    [(synth.pack77("CQ", "G4XYZ", "IO91"), 2850.0, 0.5, -5.0)])
    prev = decode_frames(first[None])[0]
    d = decode_frames(cont[None], recall=[prev], reports=True)[0]
    print("recall messages:", sum(m["recall"] for m in d), "of", len(d))
    assert any(m["recall"] for m in d) and not all(m["recall"] for m in d)
    assert all((m["report"] is None) == m["recall"] for m in d)
    # refused combinations name both settings
    rx = Receiver("", None, max_frames=1, reports=True)
    try:
        with pytest.raises(_lib.Ft8rxError, match=r"passes.*reports|reports.*passes"):
            rx.decode_frames(first[None], passes=2)
        with pytest.raises(_lib.Ft8rxError, match=r"decode_frames_arrays.*reports"):
            rx.decode_frames_arrays(first[None])
    finally:
        rx.close()
    h = _lib.Handle(max_frames=1)
    try:
        cap = _lib.packed_capacity(1)
        b0, b1 = h.pinned_bytes(cap), h.pinned_bytes(cap)
        h.set_reports(True)
        with pytest.raises(_lib.Ft8rxError, match=r"ft8rx_set_packed_output.*ft8rx_set_reports"):
            h.set_packed_output(b0.ctypes.data, b1.ctypes.data, cap, keep=(b0, b1))
        h.set_reports(False)
        h.set_packed_output(b0.ctypes.data, b1.ctypes.data, cap, keep=(b0, b1))
        with pytest.raises(_lib.Ft8rxError, match=r"ft8rx_set_reports.*ft8rx_set_packed_output"):
            h.set_reports(True)
        h.set_packed_output(None, None, 0)
    finally:
        h.close()


def test_live_path(recipe):
    """A Receiver(reports=True, audio_source=...) under the virtual clock delivers dicts with "report", equal to the batch's; so do
    Candidate.decode / check_and_package, through the probe."""
    audio = recipe[0][0]
    want = {" ".join(m["msg_tuple"]): m["report"] for m in decode_frames(audio[None], reports=True)[0]}
    assert len(want) >= 5 and all(r is not None for r in want.values())
    vt, lock, got = [0.0], threading.Lock(), []

    def hops():
        for k in range(375):
            with lock:
                vt[0] = (k + 1) * 0.04
            yield audio[480 * k:480 * k + 480]

    rx = Receiver("any", got.append, time_source=lambda: vt[0], sleep=lambda dt: _t.sleep(0.002), audio_source=hops(), early_decode_hop=None,
                  reports=True)
    try:
        deadline = _t.time() + 60
        while len(got) < len(want) and rx.thread_error is None and _t.time() < deadline:
            _t.sleep(0.01)
    finally:
        rx.stop()
    assert rx.thread_error is None
    assert {" ".join(m["msg_tuple"]): m["report"] for m in got} == want
    # the reference's own driving loop on the same frame
    got2 = []
    rx = Receiver("x", got2.append, reports=True)
    try:
        rx.audio_in.load_frame(audio)
        cands = rx.search("700101_000015", 0)
        dup = set()
        for rnd in range(8):
            for c in sorted([c for c in cands if not c.decode_result], key=lambda c: c.llr_sd, reverse=True):
                c.decode(10 + rnd)
                if c.decode_result not in (None, "stop"):
                    c.check_and_package(dup)
    finally:
        rx.close()
    assert len(got2) >= 3
    for m in got2:
        assert m["report"] == want[" ".join(m["msg_tuple"])], m
