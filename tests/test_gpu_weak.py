"""Weak mode (ft8rx_set_weak) on the GPU: the default path is untouched, k_sync3 and k_fine_weak are bit-exact
against their numpy twin (tests/weak_twin.py), a batch's fine fields equal the probe's, and weak mode decodes signals at -20 / -19 dB
that the default misses without adding false decodes on noise, on BASELINE config 1 or on the two recordings."""
import json

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import oracle as O
import weak_twin as W
from conftest import ROOT, load_golden
from pyft8_amd import _lib, synth
from pyft8_amd.receiver import Receiver, config_from_kwargs, decode_frames, frames_from_wav

pytestmark = pytest.mark.gpu
SENS_SEED = 6_000_000
# floors of weak mode's true decodes on these 64 frames x 10 signals: measured (profiles/weak_measure.json: 411 at -20 dB, 607 at
# -19 dB; the default 10 / 103) minus SENS_MARGIN.  False decodes in the set: measured 5, bound SENS_MAX_FALSE
SENS_MARGIN = 40
SENS_FLOOR = {-20.0: 411 - SENS_MARGIN, -19.0: 607 - SENS_MARGIN}
SENS_MAX_FALSE = 8
NOISE_FRAMES, NOISE_MAX_FALSE = 2048, 30      # measured 21 (the default: 0)


def sens_frame(index, snr):
    """10 random messages 240 Hz apart (+-20 Hz: >= 200 Hz), t0 uniform in [0, 1.5] s, all at snr dB (tools/weak_measure.py)."""
    rng = np.random.default_rng(SENS_SEED + index)
    sig, truth = [], []
    for k in range(10):
        msg = synth.random_message(rng)
        f0 = 300.0 + 240.0 * k + rng.uniform(-20.0, 20.0)
        t0 = rng.uniform(0.0, 1.5)
        sig.append((synth.pack77(*msg), f0, t0, snr))
        truth.append((" ".join(msg), f0))
    return synth.frame_with_signals(SENS_SEED + index, sig), truth


def score(dicts, truth):
    t = f = 0
    for ms, tr in zip(dicts, truth):
        for m in ms:
            txt = " ".join(m["msg_tuple"])
            if any(txt == x and abs(m["fHz"] - f0) < 10 for x, f0 in tr):
                t += 1
            else:
                f += 1
    return t, f


@pytest.fixture(scope="module")
def sens():
    out = {}
    for snr in (-20.0, -19.0):
        fr = [sens_frame(1000 * int(snr + 30) + i, snr) for i in range(64)]
        out[snr] = (np.stack([a for a, _ in fr]), [t for _, t in fr])
    return out


@pytest.fixture(scope="module")
def corpus():
    names = ["test_08", "test_09", "synth_000000", "synth_100000", "synth_200000"]
    audio = [load_golden(n)[0] for n in names]
    for wav in ("test_08.wav", "test_09.wav"):
        audio += list(frames_from_wav(f"{ROOT}/tests/golden/{wav}"))
    return np.stack(audio)


def _ev_sorted(ev, n):
    return np.sort(ev[:n], order=["cand", "ipass", "slot", "seq"]).tobytes()


def test_default_unchanged(corpus):
    """A handle that never had the setting and one switched on, used, and switched off give byte-identical records and events."""
    B = len(corpus)
    h0, h1 = _lib.Handle(max_frames=B), _lib.Handle(max_frames=B)
    try:
        ra, ca, ea, eca = (x.copy() for x in h0.decode_batch(corpus))
        h1.set_weak(True)
        rw, cw, _, _ = (x.copy() for x in h1.decode_batch(corpus))
        h1.set_weak(False)
        rb, cb, eb, ecb = h1.decode_batch(corpus)
        assert np.array_equal(ca, cb) and np.array_equal(eca, ecb)
        for f in range(B):
            assert ra[f, :ca[f]].tobytes() == rb[f, :cb[f]].tobytes()
            ne = min(int(eca[f]), _lib.EVENT_CAP)
            assert _ev_sorted(ea[f], ne) == _ev_sorted(eb[f], ne)
        assert rw.tobytes() != ra.tobytes()                       # the setting did act on the batch in between
    finally:
        h0.close(); h1.close()


@pytest.mark.parametrize("kind", ["default", "wide_time", "wide_build"])
def test_sync3_bitexact(sens, kind):
    """k_sync3 (ft8rx_sync_scores_weak): best score and h0 of every f0 of 16 frames equal the twin's -- default range, a time window
    wider than one SYNC3_WIN launch, and the wide build."""
    kw = dict(default={}, wide_time=dict(search_time_range=(-9.0, 12.0)), wide_build=dict(search_freq_range=(100, 5000)))[kind]
    cfg = config_from_kwargs(**kw)
    frames = np.concatenate([sens[-20.0][0][:8], sens[-19.0][0][:8]])
    h = _lib.Handle(cfg, max_frames=len(frames))
    try:
        grid = h.spectrogram(frames)
        sc, h0 = h.sync_scores(grid, cfg.f0_lo, cfg.f0_hi, weak=True)
    finally:
        h.close()
    for f in range(len(frames)):
        ts, th = W.sync3_scores(grid[f], cfg.f0_lo, cfg.f0_hi, cfg.h0_lo, cfg.h0_hi)
        assert sc[f].view(np.uint32).tolist() == ts.view(np.uint32).tolist(), (kind, f)
        assert h0[f].tolist() == th.tolist(), (kind, f)


def _compare_fine(got, want, i):
    assert got["ret"][i] == want["ret"], i
    assert (got["ttweak"][i], got["ftweak"][i], got["nsync"][i]) == (want["ttweak"], want["ftweak"], want["nsync"]), i
    assert got["sgrid"][i].tobytes() == want["sgrid"].tobytes(), i
    if want["ret"]:
        assert got["llr"][i].tobytes() == want["llr"].tobytes(), i
        assert np.float32(got["sd"][i]).tobytes() == np.float32(want["sd"]).tobytes() and got["snr"][i] == want["snr"], i


def test_fine_weak_bitexact(sens):
    """ft8rx_fine_weak on >= 2000 candidates (weak-mode search of 24 frames, plus h0 at and beyond the clamp edges and f0 = 4):
    ttweak, ftweak, nsync, grid, LLRs and sd equal the twin's bit for bit."""
    frames = np.concatenate([sens[-20.0][0], sens[-19.0][0]])
    cfg = _lib.default_config()
    ocfg = W.oracle_config()
    h = _lib.Handle(cfg, max_frames=len(frames))
    try:
        grid = h.spectrogram(frames)
        spec = h.cycle_spectrum(frames)
        trip = []
        for f in range(len(frames)):
            trip += [(f, c[0], c[1]) for c in W.search(grid[f], cfg, _lib.WEAK_SYNC_MIN_DEFAULT)[:48]]
        trip += [(0, 4, 0), (1, 5, -37), (2, 700, 86), (3, 500, -898), (4, 400, 577), (5, 300, -140), (6, 600, 221), (7, 958, 10)]
        assert len(trip) >= 2000
        t = np.array(trip, np.int32)
        got = h.fine(spec, t[:, 0], t[:, 1], t[:, 2], want_sgrid=True, weak=True)
    finally:
        h.close()
    want = W.fine_weak_many(spec, trip, ocfg)
    for i in range(len(trip)):
        _compare_fine(got, want[i], i)


def test_batch_fine_fields_match_probe(sens):
    """Every weak-mode batch record that went through fine sync (all but the ipass-0 decodes) holds the probe's fine fields."""
    frames = sens[-19.0][0][:16]
    h = _lib.Handle(max_frames=len(frames))
    try:
        h.set_weak(True)
        rec, cnt, _, _ = (x.copy() for x in h.decode_batch(frames))
        spec = h.cycle_spectrum(frames)
        sel = [(f, i) for f in range(len(frames)) for i in range(int(cnt[f]))
               if not (rec[f, i]["status"] == _lib.ST_DECODED and rec[f, i]["ipass"] == 0)]
        assert len(sel) > 100
        fr = np.array([f for f, _ in sel], np.int32)
        r = rec[fr, [i for _, i in sel]]
        got = h.fine(spec, fr, r["f0_idx"], r["h0_idx"], weak=True)
    finally:
        h.close()
    assert r["ttweak"].tolist() == got["ttweak"].tolist() and r["ftweak"].tolist() == got["ftweak"].tolist()
    assert r["nsync"].tolist() == got["nsync"].tolist()
    m = got["nsync"] > 6
    assert r["fine_sd"][m].tobytes() == got["sd"][m].astype(np.float32).tobytes()
    assert r["snr_fine"][m].tolist() == got["snr"][m].tolist()
    assert not (r["status"] == _lib.ST_STOP_FINE_SD).any() and not (rec["status"] == _lib.ST_STOP_GRID_SD).any()


def test_sensitivity(sens):
    """64 frames x 10 signals at -20 dB and at -19 dB: weak mode's true decodes reach the measured floors, false decodes stay within
    SENS_MAX_FALSE."""
    false = 0
    for snr, (frames, truth) in sens.items():
        d0 = score(decode_frames(frames), truth)
        d1 = score(decode_frames(frames, weak=True), truth)
        print(f"{snr} dB: default {d0}, weak {d1}")
        assert d1[0] >= SENS_FLOOR[snr] and d1[0] > d0[0], (snr, d0, d1)
        false += d1[1]
    assert false <= SENS_MAX_FALSE


def test_noise_false_decodes():
    """NOISE_FRAMES noise-only frames: weak mode's false decodes stay within the measured bound."""
    rx = Receiver("", None, max_frames=512, weak=True)
    n = 0
    try:
        for s in range(0, NOISE_FRAMES, 512):
            audio = np.stack([synth.frame_with_signals(5_000_000 + i, []) for i in range(s, s + 512)])
            n += sum(len(m) for m in rx.decode_frames(audio))
    finally:
        rx.close()
    print("false decodes on", NOISE_FRAMES, "noise frames:", n)
    assert n <= NOISE_MAX_FALSE


def test_config1_no_loss():
    """256 BASELINE config-1 frames: weak mode's true decodes >= the default's, false decodes per frame <= the default's + 0.05."""
    fr = [synth.make_frame(i, n_signals=50, snr_range=(-10.0, 10.0), return_truth=True) for i in range(256)]
    audio = np.stack([a for a, _ in fr])
    truth = [[(t["msg"], t["f0"]) for t in tr] for _, tr in fr]
    d0 = score(decode_frames(audio), truth)
    d1 = score(decode_frames(audio, weak=True), truth)
    print("config 1: default", d0, "weak", d1)
    assert d1[0] >= d0[0] and d1[1] / 256 <= d0[1] / 256 + 0.05


def test_real_audio():
    """test_08 / test_09: every message weak mode adds is in that cycle's WSJT-X FAST or NORM listing, and every default message it
    does not emit is in neither (measured: three such)."""
    with open(f"{ROOT}/tests/golden/wsjtx_cycles_1_2.json") as f:
        lst = json.load(f)["listings"]
    for name in ("test_08", "test_09"):
        audio = frames_from_wav(f"{ROOT}/tests/golden/{name}.wav")
        d0 = {" ".join(m["msg_tuple"]) for m in decode_frames(audio)[0]}
        d1 = {" ".join(m["msg_tuple"]) for m in decode_frames(audio, weak=True)[0]}
        ok = set(lst["FAST"][name]) | set(lst["NORM"][name])
        print(name, "default", len(d0), "weak", len(d1), "added", sorted(d1 - d0))
        print(name, "lost", sorted(d0 - d1))
        assert not ((d0 - d1) & ok) and (d1 - d0) <= ok, (sorted((d0 - d1) & ok), sorted(d1 - d0 - ok))


def test_receiver_search_and_candidate(sens):
    """Receiver.search in weak mode lists the twin's weak search; Candidate.decode takes the weak fine scan (its tweaks span beyond
    the default's +-8 / +-32) and decodes at least what the batch decodes of the first candidates."""
    frame, _ = sens[-19.0][0][0], None
    rx = Receiver("", None, weak=True)
    try:
        rx.audio_in.load_frame(frame)
        cands = rx.search("000000_000000", 0)
        width = rx.audio_in.search_grid.shape[1]
        grid = np.ones((_lib.GRID_ROWS, _lib.GRID_COLS), np.float32)          # as Receiver.search lays out the cycle's rows
        grid[1:376, :width] = rx._handle(1).spectrogram(frame[None])[0, 1:376, :width]
        want = W.search(grid, rx.cfg, _lib.WEAK_SYNC_MIN_DEFAULT)
        assert [(c.origin["f0_idx"], c.origin["h0_idx"], np.float32(c.origin["score"])) for c in cands] == \
            [(a, b, np.float32(s)) for a, b, s in want]
        spec = rx.audio_in.get_cycle_spectrum()
        c = cands[0]
        c.decode(0); c.decode(1)
        f = rx._handle(1).fine(spec[None], [0], [want[0][0]], [want[0][1]], weak=True)
        assert c.tweaks == " t:%+03d f:%+03d" % (int(f["ttweak"][0]), int(f["ftweak"][0]))
    finally:
        rx.close()


def test_refusals():
    with pytest.raises(_lib.Ft8rxError, match="weak"):
        Receiver("", None, weak=True, recall=True)
    with pytest.raises(_lib.Ft8rxError, match="msg_types"):
        Receiver("", None, weak=True, msg_types="all")
    with pytest.raises(_lib.Ft8rxError, match="my_call"):
        Receiver("", None, weak=True, my_call="K1ABC")
    audio = synth.make_frame(1, n_signals=5)[None]
    with pytest.raises(_lib.Ft8rxError, match="passes"):
        decode_frames(audio, passes=2, weak=True)
    with pytest.raises(_lib.Ft8rxError, match="weak"):
        decode_frames(audio, recall=[[]], weak=True)
    h = _lib.Handle(max_frames=1)
    try:
        h.set_weak(True)
        with pytest.raises(_lib.Ft8rxError, match="weak"):
            h._chk(h._L.ft8rx_set_msg_types(h._h, 1), "ft8rx_set_msg_types")
        with pytest.raises(_lib.Ft8rxError, match="weak"):
            h.set_ap_calls("K1ABC", None)
        buf = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        buf2 = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        with pytest.raises(_lib.Ft8rxError, match="weak"):
            h.set_packed_output(buf.data_ptr(), buf2.data_ptr(), 1 << 20)
        with pytest.raises(_lib.Ft8rxError):
            h.set_weak(True, -1.0, 40)
        with pytest.raises(_lib.Ft8rxError):
            h.set_weak(True, 148.0, 0)
    finally:
        h.close()
