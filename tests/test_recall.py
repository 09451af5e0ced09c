"""Recall decoding of stations heard 30 s earlier (ipass 8, ft8rx_set_recall), the host side: hypothesis lists (native and the numpy
twin), which entries qualify, entries from message rows and dicts, the packagers' rendering of ipass-8 records, and the ABI in
both libraries.  No GPU needed."""
import numpy as np
import pytest

from pyft8_amd import _lib, synth
from pyft8_amd import messages as M
from pyft8_amd import recall as R

REPORTS = [f"{n:+03d}" for n in range(-30, 31)]


def _entry(text, f0=200, h0=10):
    return R._entry(synth.pack77(*text), f0, h0)


def _texts(words):
    return [M.unpack(w, M.CallHashes()) for w in words]


@pytest.mark.parametrize("text", [("K1ABC", "W9XYZ", "FN42"), ("K1ABC", "W9XYZ", "-12"), ("K1ABC", "W9XYZ", "R+05"),
                                  ("K1ABC", "W9XYZ", "RR73"), ("G4ABC/P", "W9XYZ", "RRR"), ("K1ABC", "W9XYZ/R", "73")])
def test_hypotheses_of_a_call(text):
    w = synth.pack77(*text)
    words, cls = R.hypotheses(w)
    a, b = text[:2]
    want = [text] + [(a, b, x) for x in ["RRR", "RR73", "73"] + REPORTS + ["R" + r for r in REPORTS] if x != text[2]]
    assert _texts(words) == want
    assert len(words) == (126 if text[2] == "FN42" else 125) and words[0] == w
    name = lambda x: x if x in ("RRR", "RR73", "73") else "R-report" if x.startswith("R") else "report"
    assert [M.RECALL_CLASSES[c] for c in cls] == ["repeat"] + [name(t[2]) for t in want[1:]]
    # the calls' /P or /R flags and i3 stay (i3 = 2 for a /P message)
    assert all(x & 7 == w & 7 for x in words) and all((x >> 19) == (w >> 19) for x in words)
    assert _lib.recall_hypotheses(_entry(text)) == words


@pytest.mark.parametrize("text", [("CQ", "W9XYZ", "FN42"), ("QRZ", "G4ABC", "IO91"), ("DE", "K1ABC", "-05")])
def test_hypotheses_of_a_token(text):
    w = synth.pack77(*text)
    assert R.hypotheses(w) == ([w], [0])
    assert _lib.recall_hypotheses(_entry(text)) == [w]


def _i3_1(ca, cb, g15=32435, i3=1):
    return (ca << 49) | (cb << 20) | (g15 << 3) | i3


@pytest.mark.parametrize("word,why", [
    (_i3_1(M.NTOKENS + 12345, synth.pack_c28("W9XYZ")), "hashed first call"),
    (_i3_1(synth.pack_c28("K1ABC"), M.NTOKENS + 777), "hashed second call"),
    (_i3_1(500, synth.pack_c28("W9XYZ")), "CQ with a number"),
    (_i3_1(synth.pack_c28("K1ABC"), 2), "token as the sender"),
    ((123456789 << 6) | 0, "free text (i3 = 0)"),
    ((987654321 << 3) | 4, "non-standard call (i3 = 4)"),
    ((55555 << 3) | 3, "field day (i3 = 3)"),
    ((55555 << 3) | 5, "EU VHF (i3 = 5)")])
def test_skipped_entries(word, why):
    assert R.kind(word) == 0 and R.hypotheses(word) == ([], []), why
    assert _lib.recall_hypotheses(R._entry(word, 200, 10)) == [], why


def test_entry_layout():
    assert _lib.RECALL_ENTRY_DTYPE.itemsize == 24 and _lib.RECALL_MAX == 64 and _lib.M_RECALL == 6
    assert M.RECALL_CLASSES == _lib.RECALL_CLASSES


SYMBOLS = ["ft8rx_set_recall", "ft8rx_fetch_recall", "ft8rx_set_recall_gates", "ft8rx_recall_hypotheses", "ft8rx_recall_probe",
           "ft8rx_package_batch_recall"]


@pytest.mark.parametrize("wide", [False, True])
def test_abi_symbols(wide):
    L = _lib.lib(wide)
    for s in SYMBOLS:
        assert hasattr(L, s), s
    e = _entry(("K1ABC", "W9XYZ", "-12"))
    lo, hi = np.zeros(126, np.uint64), np.zeros(126, np.uint64)
    assert L.ft8rx_recall_hypotheses(e.ctypes.data, lo.ctypes.data, hi.ctypes.data) == 125


def _ladder(n=3):
    """A frame with n ladder decodes (ipass 4, fine) and their events."""
    rec = np.zeros(8, _lib.RECORD_DTYPE)
    ev = np.zeros(_lib.EVENT_CAP, _lib.EVENT_DTYPE)
    words = [synth.pack77("N0CALL", "VE3ABC", "-10"), synth.pack77("CQ", "JA1XYZ", "PM95"), synth.pack77("G4XYZ", "AA9ZZ", "R-03")][:n]
    for i, w in enumerate(words):
        r = rec[i]
        r["status"], r["ipass"], r["method"], r["n_its"] = _lib.ST_DECODED, 4, _lib.M_LDPC_B, 2
        r["f0_idx"], r["h0_idx"], r["ttweak"], r["ftweak"], r["snr_fine"] = 100 + 50 * i, 12 + i, -4, 8, -7 + i
        r["fine_sd"] = 9.0 - i
        r["msg_lo"], r["msg_hi"] = w & ((1 << 64) - 1), w >> 64
        ev[i] = (w & ((1 << 64) - 1), w >> 64, i, 4, 0, 3, 1)
    for i in range(n, 8):
        rec[i]["status"] = _lib.ST_EXHAUSTED
    return rec, ev, n, words


def _recall(texts, status=None):
    rr = np.zeros(_lib.RECALL_MAX, _lib.RECORD_DTYPE)
    for e, t in enumerate(texts):
        if t is None:
            continue                                              # a skipped entry: its record stays zero
        w = synth.pack77(*t)
        r = rr[e]
        r["status"] = _lib.ST_DECODED if status is None else status[e]
        r["ipass"], r["method"], r["ap"], r["n_its"], r["osd_hd"], r["pad2"] = 8, _lib.M_RECALL, 2, 2, 40, 80
        r["f0_idx"], r["h0_idx"], r["ttweak"], r["ftweak"], r["snr_fine"] = 600 + 10 * e, 20, 2, -8, -21
        r["msg_lo"], r["msg_hi"] = w & ((1 << 64) - 1), w >> 64
    return rr, len(texts)


def test_packagers_render_ipass8():
    """Both packagers: recall messages after the ladder's, in entry order; a text the frame has is skipped; a rejected or skipped
    entry renders nothing; notes name the step and the class; the table learns the recalled calls."""
    rec, ev, nl, words = _ladder()
    rr, rn = _recall([("K1ABC", "W9XYZ", "RR73"), ("N0CALL", "VE3ABC", "-10"), None, ("KH6ABC", "W1AW", "RR73"),
                      ("ZZ9ZZZ", "W9XYZ", "RR73")], status=[1, 1, 0, 1, _lib.ST_EXHAUSTED])
    t_py = M.CallHashes()
    py = M.package_frame(rec, 8, ev, nl, table=t_py, recall=(rr, rn))
    tn = _lib.CallHashTable()
    msgs, mcnt = _lib.package_batch_recall(rec[None], np.array([8], np.int32), ev[None], np.array([nl], np.int32), rr[None],
                                           np.array([rn], np.int32), table=tn)
    nat = M.message_dicts(msgs[0], mcnt[0], recall=True)
    want = [M.unpack(w, M.CallHashes()) for w in words] + [("K1ABC", "W9XYZ", "RR73"), ("KH6ABC", "W1AW", "RR73")]
    for out in (py, nat):
        assert [m["msg_tuple"] for m in out] == want
        assert [m["recall"] for m in out] == [False] * 3 + [True] * 2
        assert out[3]["decode_notes"] == "fine_RECALL_RR73 t:+02 f:-08" and out[3]["their_snr"] == "-21"
        assert out[3]["fHz"] == pytest.approx(3.125 * 600 - 0.5) and out[3]["tsec"] == pytest.approx(20 / 25 + 0.01)
    strip = lambda L: [{k: v for k, v in m.items() if k != "decode_completed"} for m in L]
    assert strip(py) == strip(nat)
    assert "KH6ABC" in t_py.by_call and "W1AW" in t_py.by_call and "ZZ9ZZZ" not in t_py.by_call
    t_ref = M.CallHashes()
    M.package_frame(rec, 8, ev, nl, table=t_ref)
    tn_ref = _lib.CallHashTable()
    _lib.package_batch(rec[None], np.array([8], np.int32), ev[None], np.array([nl], np.int32), table=tn_ref)
    # K1ABC, W9XYZ, KH6ABC, W1AW: four calls, three hash widths each in the native table
    assert len(t_py.by_call) == len(t_ref.by_call) + 4 and len(tn) == len(tn_ref) + 12


def test_default_rendering_unchanged():
    """Without recall results the packagers give what they gave before, and dicts have no "recall" key."""
    rec, ev, nl, _ = _ladder()
    a = M.package_frame(rec, 8, ev, nl)
    msgs, mcnt = _lib.package_batch(rec[None], np.array([8], np.int32), ev[None], np.array([nl], np.int32))
    b = M.message_dicts(msgs[0], mcnt[0])
    assert all("recall" not in m for m in a + b)
    rr, _ = _recall([])
    m2, c2 = _lib.package_batch_recall(rec[None], np.array([8], np.int32), ev[None], np.array([nl], np.int32), rr[None], np.zeros(1, np.int32))
    assert m2[0, :c2[0]].tobytes() == msgs[0, :mcnt[0]].tobytes()


def test_entries_from_rows_and_dicts():
    """Rows -> entries exactly (word, position, tweaks); dicts made from the same records land on the same grid positions."""
    rec, ev, nl, words = _ladder()
    rr, rn = _recall([("K1ABC", "W9XYZ", "RR73")])
    msgs, mcnt = _lib.package_batch_recall(rec[None], np.array([8], np.int32), ev[None], np.array([nl], np.int32), rr[None],
                                           np.array([rn], np.int32))
    e_rows = R.entries_from_rows(msgs[0], mcnt[0])
    assert len(e_rows) == 4
    allw = words + [synth.pack77("K1ABC", "W9XYZ", "RR73")]
    srcs = [rec[i] for i in range(3)] + [rr[0]]
    for e, w, r in zip(e_rows, allw, srcs):
        assert (int(e["msg_hi"]) << 64) | int(e["msg_lo"]) == w
        assert (int(e["f0_idx"]), int(e["h0_idx"]), int(e["ttweak"]), int(e["ftweak"])) == \
               (int(r["f0_idx"]), int(r["h0_idx"]), int(r["ttweak"]), int(r["ftweak"]))
    e_dicts = R.entries_from_dicts(M.message_dicts(msgs[0], mcnt[0], recall=True))
    assert e_dicts.tobytes() == e_rows.tobytes()
    # a dict of another decoder (no tweaks): the nearest grid position
    d = {"msg_tuple": ("K1ABC", "W9XYZ", "-05"), "fHz": 1000.0 + 1.4, "tsec": 0.52, "their_snr": "-10"}
    e = R.entries_from_dicts([d])
    assert (int(e[0]["f0_idx"]), int(e[0]["h0_idx"])) == (320, 13)


def test_entry_selection():
    """Non-qualifying messages are skipped silently; of the rest the RECALL_MAX with the highest SNR are kept, in their order."""
    rng = np.random.default_rng(5)
    dicts = []
    for i in range(100):
        t = synth.random_message(rng)
        dicts.append({"msg_tuple": t, "fHz": 500.0 + 10 * i, "tsec": 0.5, "their_snr": f"{i - 50:+03d}"})
    dicts.append({"msg_tuple": ("<...>", "W9XYZ", "-05"), "fHz": 900.0, "tsec": 0.5, "their_snr": "+20"})
    dicts.append({"msg_tuple": ("HELLO", "WORLD", ""), "fHz": 950.0, "tsec": 0.5, "their_snr": "+20"})
    e = R.entries_from_dicts(dicts)
    assert len(e) == _lib.RECALL_MAX
    assert [int(x["f0_idx"]) for x in e] == [int(round((500.0 + 10 * i) / 3.125)) for i in range(36, 100)]


def test_scorer_twin_on_a_clean_grid():
    """The numpy scorer on a noiseless grid of the word's own tones: the word wins at distance 0, any runner-up far behind."""
    for text in [("K1ABC", "W9XYZ", "RR73"), ("CQ", "W9XYZ", "FN42")]:
        w = synth.pack77(*text)
        g = np.full((79, 8), 0.01, np.float32)
        for s, tone in enumerate(synth.tones79(w)):
            g[s, tone] = 1.0
        r = R.score(g, w)
        assert r["word"] == w and r["hd"] == 0 and r["accept"] and r["hd2"] >= 20
        g2 = g.copy()
        wrong = synth.pack77(text[0], text[1], "RRR" if text[0] != "CQ" else "FN43")
        for s, tone in enumerate(synth.tones79(wrong)):
            g2[s] = 0.01
            g2[s, tone] = 1.0
        r2 = R.score(g2, w)
        assert (r2["word"] == wrong) == (text[0] != "CQ")
