"""Ladder kernels with more items than blocks (ft8rx_set_ladder_grid).  Every ladder kernel launches a bounded grid
and strides over a device work list; at the compiled cap of 32768 blocks nearly every block of nearly every test runs the loop body
once.  Here the cap is 1 (one block carries its state across the whole list), 3 (odd: most trips of k_fine's padded loop hit
`continue`), 8 (one block per XCD) and 61 (a prime below the list lengths: some blocks get one item more than others), on batches of
2 .. 4 frames (16 where a batch has to be cut into chunks), so that a block's second and later items -- LDS images, masks and
per-item register state reused -- decide the result.  Each configuration is held to the CPU oracle or twin where one exists, and
byte for byte (records, counts, the sorted event log, the natively packaged messages, the opt-in's own output) to the same settings at
the default cap; each test counts from the records that its batch really held more items than blocks."""
import contextlib
import hashlib

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import oracle as O
import weak_twin as W
from pyft8_amd import _lib, synth
from pyft8_amd import messages as M
from pyft8_amd.receiver import config_from_kwargs
from test_gpu_ap_calls import DX, MY, SENS_SNR, _sens_frames
from test_gpu_message_types import ALL, NEW_TYPES, expected, round_trip  # noqa: F401 -- round_trip: that module's fixture, requested here too
from test_gpu_parity import _check_frame
from test_gpu_report import _decoded
from test_gpu_weak import sens_frame

pytestmark = pytest.mark.gpu
CAPS = (1, 3, 8, 61)
EV_KEY = ["cand", "ipass", "slot", "seq"]


# ------------------------------------------------------------------------------------------------ helpers
@pytest.fixture(autouse=True)
def oracle_once(monkeypatch):
    """_check_frame decodes the frame with the oracle itself: here each (frame, config) is decoded once and reused across the caps."""
    real = O.decode_frame

    def cached(audio, cfg=None):
        key = (hashlib.sha1(np.ascontiguousarray(audio, np.int16)).digest(), bytes(cfg) if cfg is not None else None)
        if key not in _ORACLE:
            _ORACLE[key] = real(audio, cfg)
        return _ORACLE[key]
    monkeypatch.setattr(O, "decode_frame", cached)


_ORACLE, _DEFAULT, _TWIN = {}, {}, {}


@contextlib.contextmanager
def _open(cfg, n_frames, cap, setup=None):
    h = _lib.Handle(cfg, max_frames=n_frames)
    try:
        if setup:
            setup(h)
        h.set_ladder_grid(cap)
        yield h
    finally:
        h.close()


def _results(rec, cnt, ev, evc, mask=0):
    rec, cnt, ev, evc = rec.copy(), cnt.copy(), ev.copy(), evc.copy()
    msgs, mcnt = _lib.package_batch_ext(rec, cnt, ev, evc, mask) if mask else _lib.package_batch(rec, cnt, ev, evc)
    return dict(rec=rec, cnt=cnt, ev=ev, evc=evc, msgs=msgs, mcnt=mcnt)


def _run(h, audio, mask=0):
    return _results(*h.decode_batch(audio), mask=mask)


def _default(key, cfg, audio, setup=None, mask=0, extra=None):
    """The same settings at the default cap on a fresh handle, computed once per configuration and left unchanged."""
    if key not in _DEFAULT:
        with _open(cfg, len(audio), 0, setup) as h:
            r = _run(h, audio, mask)
            if extra:
                r.update(extra(h))
        _DEFAULT[key] = r
    return _DEFAULT[key]


def _same(a, b, events=True):
    assert np.array_equal(a["cnt"], b["cnt"]) and np.array_equal(a["mcnt"], b["mcnt"])
    if events:
        assert np.array_equal(a["evc"], b["evc"])
    for f in range(len(a["cnt"])):
        assert a["rec"][f, :a["cnt"][f]].tobytes() == b["rec"][f, :b["cnt"][f]].tobytes(), f
        assert a["msgs"][f, :a["mcnt"][f]].tobytes() == b["msgs"][f, :b["mcnt"][f]].tobytes(), f
        if events:
            ne = min(int(a["evc"][f]), _lib.EVENT_CAP)
            assert np.sort(a["ev"][f, :ne], order=EV_KEY).tobytes() == np.sort(b["ev"][f, :ne], order=EV_KEY).tobytes(), f


def _items(res, frames=None):
    """What the work lists of one kernel chain held, counted from its records: candidates whose ipass-0 BP attempt decoded (a lower
    bound of k_bp's list of pending attempts, which the records do not show in full), candidates that reached fine sync (k_fine*'s
    list; `far`: those beyond the frequency-domain h0 range, k_fine_td's share), candidates that reached OSD (k_osd*'s list holds ten
    attempts for each; with a-priori calls the EXHAUSTED ones of them are k_bp_ap's list, times the patterns), DECODED slots
    (k_report's list) and ipass-7 decodes."""
    frames = range(len(res["cnt"])) if frames is None else frames
    r = np.concatenate([res["rec"][f, :res["cnt"][f]] for f in frames])
    st, ip = r["status"], r["ipass"]
    dec = st == _lib.ST_DECODED
    fine = (st >= _lib.ST_STOP_COSTAS) | (dec & (ip >= 2))
    far = (r["h0_idx"] < _lib.MIN_H0_FD) | (r["h0_idx"] > _lib.MAX_H0_FD)
    return dict(bp0=int((dec & (ip == 0) & (r["method"] == _lib.M_LDPC_A)).sum()), fine=int(fine.sum()), far=int((fine & far).sum()),
                osd=int(((st == _lib.ST_EXHAUSTED) | (dec & (ip >= 5))).sum()), ap=int(((st == _lib.ST_EXHAUSTED) | (dec & (ip == 7))).sum()),
                decoded=int(dec.sum()), ipass7=int((dec & (ip == 7)).sum()))


def _claim(name, cap, items, *keys, **some):
    """The batch held more items than the largest cap has blocks, for every list in `keys`; a list given as key=caps holds fewer in this
    recipe (or the records show only a lower bound of it) and is claimed for those caps alone."""
    print(f"ladder_stride {name} cap={cap}: " + " ".join(f"{k}={v}" for k, v in items.items()))
    for k in keys:
        assert items[k] > max(CAPS), (name, k, items)
    for k, caps in some.items():
        assert items[k] > max(caps), (name, k, caps, items)


def _check_oracle(res, audio, ocfg):
    return sum(_check_frame(res["rec"][f], res["cnt"][f], res["ev"][f], res["evc"][f], audio[f], None, ocfg) for f in range(len(audio)))


@pytest.fixture(scope="module")
def ocfg():
    return O.default_config(**_lib.fft_plans())


@pytest.fixture(scope="module")
def dense4():
    return synth.make_batch(88000, 4)


@pytest.fixture(scope="module")
def dense16():
    return synth.make_batch(88100, 16)


# ------------------------------------------------------------------------------------------------ the configurations
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("streams", [1, 2])
def test_defaults(cap, streams, dense4, dense16, ocfg):
    """k_bp mode 0, k_fine, k_osd.  One stream: four frames in one chain.  Two streams: sixteen frames, the smallest batch that is cut
    into chunks (eight frames each, batch_plan.hpp), so that two chains with lists and counters of their own run side by side."""
    audio = dense4 if streams == 1 else dense16
    setup = lambda h: h.set_streams(streams)
    with _open(None, len(audio), cap, setup) as h:
        res = _run(h, audio)
    for chunk in ([range(4)] if streams == 1 else [range(0, 8), range(8, 16)]):
        _claim(f"defaults/streams={streams}", cap, _items(res, chunk), "bp0", "fine", "osd")
    assert _check_oracle(res, audio, ocfg) > 15 * len(audio)
    _same(res, _default(("defaults", streams), None, audio, setup))


@pytest.mark.parametrize("cap", CAPS)
def test_ladder_mode_1(cap, dense4, ocfg):
    """ft8rx_set_ladder_mode(1): the five-variant k_bp launch feeds k_osd's list.  The oracle's records and messages, mode 0's records
    and messages at the default cap, and mode 1's own event log at the default cap."""
    setup = lambda h: h.set_ladder_mode(1)
    with _open(None, 4, cap, setup) as h:
        res = _run(h, dense4)
    _claim("ladder_mode=1", cap, _items(res), "bp0", "fine", "osd")
    _check_oracle(res, dense4, ocfg)
    _same(res, _default(("defaults", 1), None, dense4, lambda h: h.set_streams(1)), events=False)
    _same(res, _default("ladder_mode=1", None, dense4, setup))


@pytest.fixture(scope="module")
def low4():
    return np.stack([synth.make_frame(70000 + i, n_signals=30, snr_range=(-20.0, -8.0)) for i in range(4)])


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("kw", [dict(osd_single=91, osd_double=4), dict(osd_triple=30, osd_max_hd=32)], ids=["wide_flips", "triples_gate"])
def test_osd_knobs(cap, kw, low4):
    """k_osd_wide (91 flip rows: the second flip word) and order-3 trials behind the distance gate, on low-SNR frames where OSD does
    most of the decoding; the oracle runs with the same knobs."""
    cfg = _lib.default_config(**kw)
    with _open(cfg, 4, cap) as h:
        res = _run(h, low4)
    _claim(f"osd_knobs/{kw}", cap, _items(res), "fine", "osd")
    _check_oracle(res, low4, O.default_config(**_lib.fft_plans(), **kw))
    _same(res, _default(("osd_knobs", tuple(kw.items())), cfg, low4))


@pytest.mark.parametrize("cap", CAPS)
def test_message_types(cap, round_trip):  # noqa: F811
    """msg_types = "all" (k_grid_llr_ext feeding k_bp_ext, k_osd_ext) on six frames that carry all six opt-in types: the default cap's
    bytes, and the Python model's rendering of every transmitted word, as test_round_trip_all_types checks it.  At 0 .. +8 dB few
    candidates are left to ipass-0 BP: k_bp_ext's list is claimed for the caps 1, 3 and 8."""
    audio, sent = round_trip
    cfg = config_from_kwargs(msg_types="all")
    with _open(cfg, len(audio), cap) as h:
        res = _run(h, audio, ALL)
    _claim("msg_types=all", cap, _items(res), "fine", "osd", bp0=(1, 3, 8))
    _same(res, _default("msg_types", cfg, audio, mask=ALL))
    for f, (texts, words) in enumerate(sent):
        got = M.package_frame(res["rec"][f], int(res["cnt"][f]), res["ev"][f], int(res["evc"][f]), mask=ALL)
        lines = {m["all_txt_format"].split(" ~ ")[1] for m in got if m["msg_type"] in NEW_TYPES}
        want = {expected(M._msg_text(w, M.unpack_ext(w, M.CallHashes(), ALL))) for w in words}
        assert lines == want, (f, sorted(want - lines), sorted(lines - want))


FAR_RANGE = (-30.0, 3.0)


@pytest.fixture(scope="module")
def far3():
    return synth.make_batch(61500, 3)


def _nan_attempts(audio, ocfg):
    """OSD attempts of the batch whose vector holds some, not only, NaNs -- what k_osd hands to k_osd_nan: for every candidate the
    oracle takes to OSD, its five fine LLR vectors with the AP override and the outputs BP left of them."""
    n = 0
    for a in audio:
        spec = O.cycle_spectrum(a, ocfg)
        for c in O.decode_frame(a, ocfg)["cands"]:
            if not (c.status == _lib.ST_EXHAUSTED or (c.status == _lib.ST_DECODED and c.ipass >= 5)):
                continue
            llr = O.fine(spec, c.f0_idx, c.h0_idx, ocfg)["llr"]
            for ap in range(5):
                x = O.set_ap(llr, ap)
                out = O.ldpc(x, ocfg.bp_nc0_b, ocfg.bp_iters_b)[3]
                n += sum(int(np.isnan(v).any() and not np.isnan(v).all()) for v in (x, out) if v is not None)
    return n


@pytest.mark.parametrize("cap", CAPS)
def test_far_time_range(cap, far3):
    """A search_time_range beyond -6.1 .. +8.3 s: k_fine_td takes the candidates beyond the frequency-domain h0 range, and candidates
    with h0 <= -33 reach OSD.  None of their vectors holds a NaN in this recipe (counted with the oracle and asserted: the window's
    NaN list is empty at every cap), so this test claims no cap for k_osd_nan; test_osd_nan_stage_entry strides it."""
    cfg = config_from_kwargs(sync_score_min=70, search_time_range=FAR_RANGE)
    assert cfg.h0_lo < _lib.MIN_H0_FD
    ocfg = O.default_config(**_lib.fft_plans(), sync_score_min=70.0, f0_lo=cfg.f0_lo, f0_hi=cfg.f0_hi, h0_lo=cfg.h0_lo, h0_hi=cfg.h0_hi)
    with _open(cfg, 3, cap) as h:
        res = _run(h, far3)
    items = _items(res)
    if "far_nan" not in _TWIN:
        _TWIN["far_nan"] = _nan_attempts(far3, ocfg)
    items["nan"] = _TWIN["far_nan"]
    r = np.concatenate([res["rec"][f, :res["cnt"][f]] for f in range(3)])
    items["osd_h0_le_-33"] = int(((r["h0_idx"] <= -33) & ((r["status"] == _lib.ST_EXHAUSTED) | ((r["status"] == _lib.ST_DECODED) & (r["ipass"] >= 5)))).sum())
    _claim("far_time_range", cap, items, "fine", "far", "osd", "osd_h0_le_-33")
    assert items["nan"] == 0
    _check_oracle(res, far3, ocfg)
    _same(res, _default("far", cfg, far3))


def _nan_vectors():
    """160 noisy codewords (sigma 3 on +-4: about two in three decode, many of them beyond trial 0): 128 with 1 .. 40 NaNs each
    (k_osd_nan's list: more entries than any cap here has blocks), 8 all NaN and 24 without -- the main kernel keeps those."""
    rng = np.random.default_rng(61)
    x = np.empty((160, 174), np.float32)
    for k in range(160):
        cw = synth.encode174(synth.pack77(*synth.random_message(rng)))
        x[k] = [4.0 if (cw >> (173 - i)) & 1 else -4.0 for i in range(174)]
    x += (rng.standard_normal(x.shape) * 3.0).astype(np.float32)
    for k in range(128):
        x[k, rng.choice(174, 1 + k % 40, replace=False)] = np.nan
    x[128:136] = np.nan
    x[136:144, :29] = np.where(rng.random((8, 29)) < 0.5, 5.0, -5.0)            # AP-style exact ties
    return x


@pytest.mark.parametrize("cap", CAPS)
def test_osd_nan_stage_entry(cap):
    """k_osd_nan / k_osd_nan_wide with more list entries than blocks.  The chain's NaN list is almost always empty, so the list comes
    from ft8rx_osd_ext: its main kernel keeps one block per vector and leaves the 128 vectors with some NaNs to the NaN kernel, which
    runs min(512, cap) blocks.  Outcome, word and trial index equal the oracle's (computed once), as in test_osd_ties_and_nans."""
    x = _nan_vectors()
    with _open(None, 1, cap) as h:
        for s, d in [(30, 2), (91, 4)]:
            if ("nan", s, d) not in _TWIN:
                _TWIN["nan", s, d] = [O.osd(v, s, d) for v in x]
            want = _TWIN["nan", s, d][:128]
            assert sum(w[0] for w in want) > max(CAPS) and sum(w[0] and w[2] > 0 for w in want) > 20      # decodes, and not only order-0 ones
            ok, lo, hi, trial = h.osd(x, s, d)
            for k, (w_ok, w_bits, w_trial, _) in enumerate(_TWIN["nan", s, d]):
                assert bool(ok[k]) == w_ok and (not w_ok or (((int(hi[k]) << 64) | int(lo[k])) == w_bits and trial[k] == w_trial)), (s, d, k)


@pytest.fixture(scope="module")
def weak8():
    return np.stack([sens_frame(11000 + i, -19.0)[0] for i in range(8)])


@pytest.mark.parametrize("cap", CAPS)
def test_weak(cap, weak8):
    """Weak mode on eight frames of ten signals at -19 dB: k_fine_weak, then OSD behind the weak distance gate.  The default cap's
    bytes; the fine fields of the first six candidates of each frame that went through fine sync equal the numpy twin's on the GPU's
    own cycle spectrum (test_fine_weak_bitexact's twin)."""
    setup = lambda h: h.set_weak(True)
    with _open(None, 8, cap, setup) as h:
        res = _run(h, weak8)
        if "weak" not in _TWIN:
            spec = h.cycle_spectrum(weak8)
            trip = []
            for f in range(8):
                r = res["rec"][f, :res["cnt"][f]]
                went = np.nonzero(~((r["status"] == _lib.ST_DECODED) & (r["ipass"] == 0)))[0][:6]
                trip += [(f, int(i), int(r[i]["f0_idx"]), int(r[i]["h0_idx"])) for i in went]
            _TWIN["weak"] = (trip, W.fine_weak_many(spec, [(f, f0, h0) for f, _, f0, h0 in trip], W.oracle_config()))
    _claim("weak", cap, _items(res), "fine", "osd")
    _same(res, _default("weak", None, weak8, setup))
    trip, twin = _TWIN["weak"]
    assert len(trip) == 48
    for (f, i, f0, h0), t in zip(trip, twin):
        r = res["rec"][f, i]
        assert (int(r["f0_idx"]), int(r["h0_idx"])) == (f0, h0)
        assert (int(r["ttweak"]), int(r["ftweak"]), int(r["nsync"])) == (t["ttweak"], t["ftweak"], t["nsync"]), (f, i)
        if t["nsync"] > 6:
            assert np.float32(r["fine_sd"]).tobytes() == np.float32(t["sd"]).tobytes() and int(r["snr_fine"]) == t["snr"], (f, i)


AP_WORDS = [synth.pack77(MY, DX, "RR73"), synth.pack77(MY, DX, "73"), synth.pack77(MY, DX, "RRR"), synth.pack77(MY, DX, "-15"),
            synth.pack77("CQ", DX, "FN42"), synth.pack77(MY, "G4ABC", "-07")]


@pytest.fixture(scope="module")
def ap28(dense4):
    """Four dense frames (their EXHAUSTED candidates fill ipass 7's lists) and the 24 six-word frames at -19 dB on which
    test_combinations_and_refusals finds ipass-7 decodes."""
    return np.concatenate([dense4, _sens_frames(24, SENS_SNR, AP_WORDS, seed0=40)])


@pytest.mark.parametrize("cap", CAPS)
def test_ap_calls(cap, ap28):
    """ipass 7 with both calls set, 28 frames in one chain: k_bp_ap strides over (EXHAUSTED candidates x 6 patterns), k_osd_ap over the
    partial patterns BP left undecided (up to three per candidate; the list's length cannot be read back, its candidates are
    counted).  The default cap's bytes, and ft8rx_ap_calls_probe at the same small cap gives frame 0's candidates the batch's outcome."""
    def setup(h):
        h.set_streams(1)
        h.set_ap_calls(MY, DX)
    with _open(None, 28, cap, setup) as h:
        res = _run(h, ap28)
        r = res["rec"][0, :res["cnt"][0]]
        sel = np.nonzero((r["status"] == _lib.ST_EXHAUSTED) | ((r["status"] == _lib.ST_DECODED) & (r["ipass"] == 7)))[0]
        fo = h.fine(h.cycle_spectrum(ap28[:1]), np.zeros(len(sel), np.int32), r["f0_idx"][sel], r["h0_idx"][sel])
        prec, _, _ = h.ap_calls_probe(fo["llr"])
    items = _items(res)
    _claim("ap_calls", cap, items, "fine", "osd", "ap")
    assert items["ipass7"] >= 1 and len(sel) > 8 and (fo["ret"] == 1).all()
    _same(res, _default("ap_calls", None, ap28, setup))
    for key in ("status", "ipass", "ap", "method", "n_its", "msg_lo", "msg_hi", "osd_hd"):
        want = r[key][sel] * (r["status"][sel] == _lib.ST_DECODED).astype(r[key].dtype) if key != "status" else r["status"][sel]
        assert np.array_equal(prec[key], want), key


@pytest.mark.parametrize("cap", CAPS)
def test_reports(cap, dense4):
    """ft8rx_set_reports: k_report strides over the DECODED slots.  fetch_reports' bytes equal the default cap's, and the probe at the
    same small cap returns the batch's bytes for every DECODED record."""
    setup = lambda h: h.set_reports(True)
    with _open(None, 4, cap, setup) as h:
        res = _run(h, dense4)
        rp = h.fetch_reports(4)
        who = _decoded(res)
        r = [res["rec"][f, i] for f, i in who]
        pr = h.report_probe(h.cycle_spectrum(dense4), [f for f, _ in who], [x["f0_idx"] for x in r], [x["h0_idx"] for x in r],
                            [x["ttweak"] for x in r], [x["ftweak"] for x in r], [(int(x["msg_hi"]) << 64) | int(x["msg_lo"]) for x in r])
    _claim("reports", cap, _items(res), "decoded")
    ref = _default("reports", None, dense4, setup, extra=lambda h: dict(rp=h.fetch_reports(4)))
    _same(res, ref)
    assert rp.tobytes() == ref["rp"].tobytes()
    batch = np.array([rp[f, i] for f, i in who], _lib.REPORT_DTYPE)
    assert pr.tobytes() == batch.tobytes() and (batch["flags"] & _lib.RP_MEASURED).all()


@pytest.mark.parametrize("cap", CAPS)
def test_deep_layouts_wide_build(cap):
    """max_cands = 1024 on the wide build, two frames searched to 4000 Hz at sync_score_min = 30: the deep per-candidate layouts, ten
    bits of candidate index in every work-list id, and candidates beyond index 512 on the fine and OSD lists.  The low threshold
    leaves few ipass-0 BP decodes and few deep candidates for OSD: those two are claimed for the caps 1, 3 and 8."""
    audio = synth.make_batch(64100, 2, n_signals=60, snr_range=(-14.0, 6.0))
    cfg = config_from_kwargs(sync_score_min=30, max_cands=1024, search_freq_range=[100, 4000])
    ocfg = O.default_config(**_lib.fft_plans(), sync_score_min=30.0, max_cands=1024, f0_lo=cfg.f0_lo, f0_hi=cfg.f0_hi)
    with _open(cfg, 2, cap) as h:
        assert h.wide
        res = _run(h, audio)
    assert (res["cnt"] > 512).all(), res["cnt"]
    _claim("deep_layouts", cap, _items(res), "fine", "osd", bp0=(1, 3, 8))
    _claim("deep_layouts beyond 512", cap, _items(dict(rec=res["rec"][:, 512:], cnt=res["cnt"] - 512)), "fine", osd=(1, 3, 8))
    _check_oracle(res, audio, ocfg)
    _same(res, _default("deep", cfg, audio))


# ------------------------------------------------------------------------------------------------ the setting itself
def test_refusals_and_default_again(dense4):
    """Caps outside [0, LADDER_GRID_CAP] are refused by name and range and leave the setting as it was; 0 after a small cap gives the
    default's results again, and so does the compiled cap given explicitly."""
    ref = _default(("defaults", 1), None, dense4, lambda h: h.set_streams(1))
    with _open(None, 4, 3) as h:
        for bad in (-1, _lib.LADDER_GRID_CAP + 1):
            with pytest.raises(_lib.Ft8rxError, match=rf"ft8rx_set_ladder_grid: cap {bad} outside \[0, {_lib.LADDER_GRID_CAP}\]"):
                h.set_ladder_grid(bad)
        _same(_run(h, dense4), ref)
        h.set_ladder_grid(0)
        _same(_run(h, dense4), ref)
        h.set_ladder_grid(_lib.LADDER_GRID_CAP)
        _same(_run(h, dense4), ref)


def test_cap_change_between_free_running_batches(dense16):
    """Two batches enqueued back to back on free-running chunk streams, the cap changed in between (the setter waits for the first):
    each gets the results of a fresh handle at the default cap."""
    other = np.ascontiguousarray(dense16[::-1])
    setup = lambda h: h.set_streams(2)
    ref = _default(("defaults", 2), None, dense16, setup)
    with _open(None, 16, 3, setup) as h:
        h.enqueue_host(dense16)
        h.set_ladder_grid(61)
        h.enqueue_host(other)
        first, second = _results(*h.fetch(16)), _results(*h.fetch(16))
    _same(first, ref)
    _same({k: v[::-1] for k, v in second.items()}, ref)


def test_same_batch_twice_at_cap_1(dense4):
    """The same batch twice through one handle whose every ladder kernel is a single block: nothing a launch leaves in LDS or in
    device globals reaches the next."""
    with _open(None, 4, 1) as h:
        a, b = _run(h, dense4), _run(h, dense4)
    _same(a, b)
    _same(a, _default(("defaults", 1), None, dense4, lambda h: h.set_streams(1)))
