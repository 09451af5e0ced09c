"""A-priori decoding with the operator's own and the DX station's calls (ipass 7, ft8rx_set_ap_calls) on the GPU: the default is
untouched, the reference's ladder keeps every record, the step finds more of the messages it is meant for, it does not invent
them from noise or from other stations' traffic, and every ipass-7 record is reproduced by the single-vector entry points."""
import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

from conftest import ROOT, load_golden
from pyft8_amd import _lib, synth
from pyft8_amd import messages as M
from pyft8_amd.receiver import Receiver, ap_calls_attempts, decode_frames, frames_from_wav

pytestmark = pytest.mark.gpu
MY, DX = "K1ABC", "W9XYZ"
SENS_SNR = -19.0                    # where the default decodes a minority of these messages (profiles/ap_calls_measure.json)
SENS_WORDS = [synth.pack77(MY, DX, "RR73"), synth.pack77(MY, DX, "-15"), synth.pack77("CQ", DX, "FN42")]


def _arrays(audio, my=None, dx=None, clear=False, max_hd=None):
    h = _lib.Handle(max_frames=len(audio))
    try:
        if max_hd is not None:
            h.set_ap_max_hd(max_hd)
        if my or dx or clear:
            h.set_ap_calls(my or MY, dx or DX) if clear else h.set_ap_calls(my, dx)
        if clear:
            h.set_ap_calls(None, None)
        return h.decode_batch(audio)
    finally:
        h.close()


def _ev_sorted(ev, n):
    return np.sort(ev[:n], order=["cand", "ipass", "slot", "seq"]).tobytes()


@pytest.fixture(scope="module")
def corpus():
    names = ["test_08", "test_09", "synth_000000", "synth_100000", "synth_200000"]
    audio = [load_golden(n)[0] for n in names]
    for wav in ("test_08.wav", "test_09.wav"):
        audio += list(frames_from_wav(f"{ROOT}/tests/golden/{wav}"))
    return np.stack(audio)


def test_default_unchanged(corpus):
    """Calls unset -- never set, or set and cleared again -- records, events and messages are byte-identical."""
    a = _arrays(corpus)
    b = _arrays(corpus, clear=True)
    (ra, ca, ea, eca), (rb, cb, eb, ecb) = a, b
    assert np.array_equal(ca, cb) and np.array_equal(eca, ecb)
    for f in range(len(corpus)):
        assert ra[f, :ca[f]].tobytes() == rb[f, :cb[f]].tobytes()
        ne = min(int(eca[f]), _lib.EVENT_CAP)
        assert _ev_sorted(ea[f], ne) == _ev_sorted(eb[f], ne)
    ma, na = _lib.package_batch(*a)
    mb, nb = _lib.package_batch(*b)
    assert ma.tobytes() == mb.tobytes() and na.tobytes() == nb.tobytes() and na.sum() > 0
    d0, d1 = decode_frames(corpus), decode_frames(corpus, my_call=None, dx_call="")
    strip = lambda L: [[{k: v for k, v in m.items() if k != "decode_completed"} for m in f] for f in L]
    assert strip(d0) == strip(d1) and all("ap" not in m for f in d0 for m in f)


def _check_superset(a, b):
    (ra, ca, _, _), (rb, cb, _, _) = a, b
    assert np.array_equal(ca, cb)
    new = 0
    for f in range(len(ca)):
        for i in range(ca[f]):
            x, y = ra[f, i], rb[f, i]
            if x["status"] == _lib.ST_DECODED or y["ipass"] != 7 or y["status"] != _lib.ST_DECODED:
                assert x.tobytes() == y.tobytes(), (f, i)
            else:
                assert x["status"] == _lib.ST_EXHAUSTED and 5 <= y["ap"] <= 10
                new += 1
    return new


def test_superset_invariant(corpus):
    """Calls set: every candidate the reference's ladder decodes keeps its record byte for byte; the new decodes are all ipass 7."""
    _check_superset(_arrays(corpus), _arrays(corpus, MY, DX))
    audio = synth.make_batch(0, 16)                                     # config-1 synthetic frames
    _check_superset(_arrays(audio), _arrays(audio, "VE3ABC", "G4XYZ"))
    _check_superset(_arrays(audio), _arrays(audio, MY, None))


def _sens_frames(n, snr, words=SENS_WORDS, seed0=0):
    return np.stack([synth.frame_from_words(seed0 + i, words, snr_range=(snr, snr)) for i in range(n)])


def _hits(dicts, words):
    """per word: frames where its text was decoded within 15 Hz of where it was sent"""
    texts = [" ".join(M.unpack(w, M.CallHashes())) for w in words]
    out = np.zeros(len(words), int)
    for f in dicts:
        for k, t in enumerate(texts):
            f0 = 300.0 + 2400.0 * (k + 0.5) / len(words)
            out[k] += any(" ".join(m["msg_tuple"]) == t and abs(m["fHz"] - f0) < 15 for m in f)
    return out


@pytest.fixture(scope="module")
def sens():
    audio = _sens_frames(64, SENS_SNR)
    d0 = decode_frames(audio)
    d1 = decode_frames(audio, my_call=MY, dx_call=DX)
    rec = _arrays(audio, MY, DX)
    return audio, d0, d1, rec


def test_sensitivity(sens):
    """MY DX RR73, MY DX -15, CQ DX FN42 at a fixed low SNR: with the calls set strictly more of them decode at the right origin."""
    _, d0, d1, _ = sens
    h0, h1 = _hits(d0, SENS_WORDS), _hits(d1, SENS_WORDS)
    print("default", h0.tolist(), "ap", h1.tolist(), "of", len(d0))
    assert (h1 >= h0).all() and h1.sum() >= h0.sum() + 4, (h0, h1)
    assert all(m["ap"] in M.AP_NAMES + M.AP_CALL_NAMES for f in d1 for m in f)


def test_wrong_hypothesis():
    """DX sends MY DX -12 at low SNR: never rendered as RRR / 73 / RR73.  Third-party traffic is never rendered with MY or DX."""
    audio = _sens_frames(32, SENS_SNR, [synth.pack77(MY, DX, "-12")] * 2 + [synth.pack77("K9AAA", "W1BBB", "RR73")], seed0=500)
    for f in decode_frames(audio, my_call=MY, dx_call=DX):
        for m in f:
            t = m["msg_tuple"]
            if t[:2] == (MY, DX):
                assert t[2] not in ("RRR", "73", "RR73"), m
            else:
                assert MY not in t and DX not in t, m


def test_noise_gives_no_ipass7():
    """2048 device-synthesised noise-only frames with both calls set: no ipass-7 decode."""
    B = 256
    h = _lib.Handle(max_frames=B)
    h.set_ap_calls(MY, DX)
    d = torch.empty((B, synth.NFRAME), dtype=torch.int16, device="cuda")
    n7 = 0
    try:
        for k in range(2048 // B):
            h.synth_frames(d.data_ptr(), 10_000_000 + k * B, B, n_signals=0)
            torch.cuda.synchronize()
            h.enqueue(d.data_ptr(), B)
            rec, cnt, _, _ = h.fetch(B)
            for f in range(B):
                r = rec[f, :cnt[f]]
                n7 += int(((r["status"] == _lib.ST_DECODED) & (r["ipass"] == 7)).sum())
    finally:
        h.close()
    assert n7 == 0


def test_exactness(sens):
    """Every ipass-7 record is reproduced by ft8rx_fine + the pattern in numpy + ft8rx_ldpc / ft8rx_osd + the distance in numpy
    (receiver.ap_calls_attempts, which Candidate.decode runs for ipass 7)."""
    audio, _, _, (rec, cnt, _, _) = sens
    cfg = _lib.default_config()
    bits, mask = _lib.ap_patterns(MY, DX)
    h = _lib.Handle(max_frames=1)
    n = 0
    import threading
    lock = threading.RLock()
    try:
        for f in range(len(audio)):
            r7 = [r for r in rec[f, :cnt[f]] if r["status"] == _lib.ST_DECODED and r["ipass"] == 7]
            if not r7:
                continue
            spec = h.cycle_spectrum(audio[f])
            for r in r7:
                fo = h.fine(spec, [0], [int(r["f0_idx"])], [int(r["h0_idx"])])
                assert fo["ret"][0] == 1
                got = ap_calls_attempts(h, cfg, fo["llr"][0], bits, mask, _lib.AP_MAX_HD_DEFAULT, lock, synth)
                word = (int(r["msg_hi"]) << 64) | int(r["msg_lo"])
                assert got == (int(r["ap"]), word, int(r["osd_hd"]), int(r["method"])), (f, got, r)
                n += 1
    finally:
        h.close()
    assert n > 0


def test_refusals():
    with pytest.raises(_lib.Ft8rxError, match="my_call"):
        Receiver("", None, my_call="K1abc")
    with pytest.raises(_lib.Ft8rxError, match="dx_call"):
        Receiver("", None, dx_call="<K1ABC>")
    with pytest.raises(_lib.Ft8rxError, match="msg_types"):
        Receiver("", None, my_call=MY, msg_types="all")
    rx = Receiver("", None, my_call=MY, dx_call=DX)
    try:
        audio = np.zeros((1, synth.NFRAME), np.int16)
        with pytest.raises(_lib.Ft8rxError, match="passes"):
            rx.decode_frames(audio, passes=2)
        with pytest.raises(_lib.Ft8rxError):
            rx._handle(1).set_packed_output(1, 2, 1 << 20)
        rx.set_ap_calls(None, None)
        assert rx.decode_frames(audio) == [[]]
        rx.set_ap_calls(DX, MY)
        assert rx._h.ap_calls == (DX, MY)
    finally:
        rx.close()


def test_candidate_decode_matches_batch(sens):
    """The reference-style per-candidate loop (Receiver.search + Candidate.decode, receiver.py:389-398) with the calls set reaches
    ipass 7 and decodes exactly the candidates the batch path decodes there, with the same pattern, word and distance."""
    audio, _, _, (rec, cnt, _, _) = sens
    rx = Receiver("x", None, my_call=MY, dx_call=DX)
    n7 = 0
    try:
        for f in range(16):
            want = {(int(r["f0_idx"]), int(r["h0_idx"])): (int(r["ap"]), (int(r["msg_hi"]) << 64) | int(r["msg_lo"]), int(r["osd_hd"]))
                    for r in rec[f, :cnt[f]] if r["status"] == _lib.ST_DECODED and r["ipass"] == 7}
            rx.audio_in.load_frame(audio[f])
            cands = rx.search("700101_000015", 0, range(*rx.audio_in.search_f0_idx_range))
            for rnd in range(8):
                for c in sorted([c for c in cands if not c.decode_result], key=lambda c: c.llr_sd, reverse=True):
                    c.decode(10 + rnd)
            got = {(c.origin["f0_idx"], c.origin["h0_idx"]): (c.ap_result["ap"], c.ap_result["word"], c.ap_result["osd_hd"])
                   for c in cands if getattr(c, "ap_result", None)}
            assert got == want, f
            n7 += len(got)
    finally:
        rx.close()
    assert n7 > 0


def _crafted_llrs(word, flips, seed, known):
    """Fine LLRs of `word`'s codeword at |4|, with `flips` weak (|0.5|) wrong bits outside the positions in `known`."""
    rng = np.random.default_rng(seed)
    cw = synth.encode174(word)
    x = np.array([4.0 if (cw >> (173 - i)) & 1 else -4.0 for i in range(174)], np.float32)
    free = np.array([i for i in range(174) if not known[i]])
    pos = rng.choice(free, flips, replace=False)
    x[pos] = -0.5 * np.sign(x[pos])
    return x


def test_bp_valid_word_beyond_gate_ends_the_pattern():
    """BP_B finds a valid word whose distance exceeds ap_max_hd: the pattern is not accepted and OSD does not run on it (no
    slot-2 ap + 1 event).  Vectors near the gate, inside it, and with NaNs: the batch's ipass-7 kernels (ft8rx_ap_calls_probe) and
    receiver.ap_calls_attempts (single-vector entry points, Candidate.decode's path) give the same record."""
    import threading
    cfg = _lib.default_config()
    bits, mask = _lib.ap_patterns(MY, DX)
    w = synth.pack77(MY, DX, "-15")
    known6 = mask[1].astype(bool)
    vecs = [_crafted_llrs(w, n, 100 + n, known6) for n in (20, 30, 38, 42, 46, 50, 54, 60)]
    nanv = _crafted_llrs(w, 30, 7, known6)
    nanv[np.nonzero(~known6)[0][:3]] = np.nan
    vecs.append(nanv)
    h = _lib.Handle(max_frames=1)
    lock = threading.RLock()
    beyond = 0
    try:
        h.set_ap_calls(MY, DX)
        rec, ev, ne = h.ap_calls_probe(np.stack(vecs))
        ev = ev[:min(ne, _lib.EVENT_CAP)]
        for i, x in enumerate(vecs):
            e = ev[ev["cand"] == i]
            words = {(int(a["slot"]), (int(a["msg_hi"]) << 64) | int(a["msg_lo"])) for a in e}
            hard = (np.nan_to_num(x) > 0)
            cw = synth.encode174(w)
            hd = sum(((cw >> (173 - k)) & 1) != hard[k] for k in range(174))
            if (12, w) in words and hd > _lib.AP_MAX_HD_DEFAULT:     # BP of "MY DX ???" met the true word beyond the gate
                beyond += 1
                assert not (e["slot"] == 13).any(), i                 # ... and no OSD followed
                assert not (e["slot"] == 11).any() or (10, w) not in words, i
            got = ap_calls_attempts(h, cfg, x, bits, mask, _lib.AP_MAX_HD_DEFAULT, lock, synth)
            r = rec[i]
            if got is None:
                assert r["status"] == _lib.ST_EXHAUSTED, (i, r)
            else:
                word = (int(r["msg_hi"]) << 64) | int(r["msg_lo"])
                assert r["status"] == _lib.ST_DECODED and r["ipass"] == 7, (i, got)
                assert got == (int(r["ap"]), word, int(r["osd_hd"]), int(r["method"])), (i, got, r)
        assert rec[0]["status"] == _lib.ST_DECODED and int(rec[0]["ap"]) == 5      # 20 flips: inside the gate, MY ??? wins the tie
        assert beyond >= 2
    finally:
        h.close()


def test_exhausted_candidates_match_twin(sens):
    """Every candidate the reference ladder leaves EXHAUSTED -- on sensitivity frames and on dense config-1 frames -- gets the same
    ipass-7 outcome, decoded or not, from the batch and from receiver.ap_calls_attempts."""
    import threading
    audio = np.concatenate([sens[0][:8], synth.make_batch(0, 2)])
    r_def, (rec, cnt, _, _) = _arrays(audio)[0], _arrays(audio, MY, DX)
    cfg = _lib.default_config()
    bits, mask = _lib.ap_patterns(MY, DX)
    h = _lib.Handle(max_frames=1)
    lock = threading.RLock()
    n = 0
    try:
        for f in range(len(audio)):
            spec = h.cycle_spectrum(audio[f])
            for i in range(cnt[f]):
                if r_def[f, i]["status"] != _lib.ST_EXHAUSTED:
                    continue
                r = rec[f, i]
                fo = h.fine(spec, [0], [int(r["f0_idx"])], [int(r["h0_idx"])])
                got = ap_calls_attempts(h, cfg, fo["llr"][0], bits, mask, _lib.AP_MAX_HD_DEFAULT, lock, synth)
                if got is None:
                    assert r["status"] == _lib.ST_EXHAUSTED, (f, i)
                else:
                    assert got == (int(r["ap"]), (int(r["msg_hi"]) << 64) | int(r["msg_lo"]), int(r["osd_hd"]), int(r["method"])), (f, i)
                n += 1
    finally:
        h.close()
    assert n > 20
