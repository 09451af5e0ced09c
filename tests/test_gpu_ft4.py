"""FT4 on the GPU (csrc/kernels/ft4.hpp) against its float64 twin pyft8_amd/ft4.py on the fixtures of
tests/ft4_cases.py: the grid, the search, the demodulator on crafted candidates, the shared back end on raw vectors, the whole path
through Receiver, what FT4 leaves alone, and the refusals.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import ft4_cases as cases
from pyft8_amd import _lib, ft4, synth
from pyft8_amd.receiver import Receiver, decode_frames_ft4

pytestmark = pytest.mark.gpu
# The grid against the twin, per row (ft4_cases.grid_errors), over the 6-signal, the all-zero and the clipped frame; asserted at 4 x the
# worst value of the first run on an MI355X, rounded up to one digit (profiles/ft4_notes.md):
#   power  max |P - P64| / max P64: measured 5.202e-7 (the 6-signal frame, row 591, bin 255; the clipped frame 4.445e-7, row 2, bin 119)
#   amp    max |sqrt P - sqrt P64| / sqrt(sum P64): measured 1.458e-7 (the clipped frame, row 320; the 6-signal frame 9.404e-8, row 42)
GRID_BOUND = 3e-6
AMP_BOUND = 6e-7
# The demodulator against the twin over the 65 crafted candidates: the winner's metric, relative (measured 1.622e-7), and
# max |llr - twin| / max |llr| (measured 2.617e-7); asserted at 4 x, rounded up.
METRIC_BOUND = 7e-7
LLR_BOUND = 2e-6


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle(max_frames=3)
    yield h
    h.close()


# ----------------------------------------------------------------------------- 5. grid
def test_grid_against_the_twin(handle):
    audio, P64 = cases.grid_frames()
    db, P = handle.ft4_grid(audio, want_power=True)
    assert db.shape == P.shape == (3, ft4.ROWS, ft4.COLS) and db.dtype == np.float32
    for f, name in enumerate(("six signals", "all zero", "clipped")):
        power, amp = cases.grid_errors(P[f], P64[f])
        r, ra = int(power.argmax()), int(amp.argmax())
        print(f"ft4 grid {name}: power {power.max():.3e} (row {r}, bin {int(np.abs(P[f, r] - P64[f, r]).argmax())}), amp {amp.max():.3e} (row {ra})")
        assert power.max() <= GRID_BOUND and amp.max() <= AMP_BOUND
    assert not P[1].any() and np.all(db[1] == -240.0)                       # the all-zero frame: exact zeros, the dB floor
    want = 10.0 * np.log10(np.maximum(P.astype(np.float64), 1e-24))         # the dB values are those of the kernel's own powers
    assert np.abs(db - want).max() <= 2e-5
    assert np.array_equal(handle.ft4_grid(audio[:1]), db[:1])               # a frame alone: the same bits


# ----------------------------------------------------------------------------- 6. search
def _search_case(handle, index, f0r, h0r, max_cands, sync_min):
    P64, db64 = cases.six_grid(index)
    cands, best, bh, S = cases.twin_search(index, *f0r, *h0r, sync_min, max_cands)
    bound = cases.score_bound_map(P64, AMP_BOUND, *f0r, *h0r)
    return cands, best, bh, bound


@pytest.mark.parametrize("max_cands", [4, 256])
def test_search_against_the_twin(max_cands):
    f0r, h0r, sm = cases.F0_RANGE, cases.H0_RANGE, cases.SEARCH_SYNC_MIN
    h = _lib.Handle(_lib.default_config(max_cands=max_cands), max_frames=3)
    try:
        h.ft4_set(sync_min=sm)
        audio = np.stack([cases.six(i)[0] for i in cases.SIX])
        grid = h.ft4_grid(audio)
        f0, h0, sc, cnt, bs, bhg = h.ft4_sync(grid, want_best=True)
        for f, index in enumerate(cases.SIX):
            cands, best, bh, bound = _search_case(h, index, f0r, h0r, max_cands, sm)
            # the fixture first: no decision of the twin's lies closer than 100 x the bound, so a near-tie is a fixture fault
            margin = cases.search_margin(cands, best, bh, bound, f0r[0], h0r[0], sm, max_cands)
            print(f"ft4 search frame {index} max_cands {max_cands}: {len(cands)} candidates, margin {margin:.0f} x the bound")
            assert margin >= 100.0 and len(cands) == min(6, max_cands)
            n = int(cnt[f])
            assert [(int(a), int(b)) for a, b in zip(f0[f, :n], h0[f, :n])] == [(c[0], c[1]) for c in cands]
            for k, c in enumerate(cands):
                b = bound[c[0] - f0r[0], c[1] - h0r[0]]
                assert abs(float(sc[f, k]) - c[2]) <= b + abs(c[2]) * 2.0 ** -23, (c, sc[f, k], b)      # + the score's own float32 rounding
            # the per-bin maxima: within the larger of the two positions' bounds wherever that is finite
            bb = np.maximum(bound[np.arange(len(best)), bh - h0r[0]], bound[np.arange(len(best)), bhg[f] - h0r[0]])
            ok = np.isfinite(bb)
            assert ok.mean() > 0.99 and np.all(np.abs(bs[f][ok] - best[ok]) <= bb[ok] + np.abs(best[ok]) * 2.0 ** -23)
    finally:
        h.close()


def test_search_in_a_one_bin_range(handle):
    """the range restricted to one f0 bin and one h0: the strongest planted signal's"""
    index = cases.SIX[0]
    f0, h0, score = cases.twin_search(index, *cases.F0_RANGE, *cases.H0_RANGE, cases.SEARCH_SYNC_MIN, 256)[0][0]
    handle.ft4_set(sync_min=cases.SEARCH_SYNC_MIN)
    handle.ft4_set_range(f0, f0 + 1, h0, h0 + 1)
    try:
        got = handle.ft4_sync(handle.ft4_grid(cases.six(index)[0]), want_best=True)
        want = ft4.search(cases.six_grid(index)[1], f0, f0 + 1, h0, h0 + 1, cases.SEARCH_SYNC_MIN, 256)
        assert want == [(f0, h0, score)] and int(got[3][0]) == 1 and (int(got[0][0, 0]), int(got[1][0, 0])) == (f0, h0)
        bound = cases.score_bound_map(cases.six_grid(index)[0], AMP_BOUND, f0, f0 + 1, h0, h0 + 1)[0, 0] + abs(score) * 2.0 ** -23
        assert got[4].shape == (1, 1) and abs(float(got[2][0, 0]) - score) <= bound and int(got[5][0, 0]) == h0
        handle.ft4_set_range(f0 + 2, f0 + 3, h0, h0 + 1)                    # one tone off: the score is far below the threshold
        assert int(handle.ft4_sync(handle.ft4_grid(cases.six(index)[0]))[3][0]) == 0
        with pytest.raises(_lib.Ft8rxError, match="ft8rx_ft4_set_range"):
            handle.ft4_set_range(0, 572, 0, 1)
    finally:
        handle.ft4_set_range()
        handle.ft4_set()


# ----------------------------------------------------------------------------- 7. demodulator
@pytest.mark.parametrize("n", [1, 3, 65])
def test_demod_against_the_twin(handle, n):
    audio, cands = cases.demod_candidates(n)
    got = handle.ft4_demod(audio, [c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands])
    assert np.isfinite(got["llr"]).all()
    worst_m, worst_l = 0.0, 0.0
    for i, c in enumerate(cands):
        tw = cases.twin_demod(*c)
        m = np.sort(tw["metrics"].ravel())
        # the fixture first: the twin's best two trials lie further apart than the metric's float32 error, so no candidate is excused ...
        assert m[-1] - m[-2] > 2.0 * METRIC_BOUND * m[-1] or m[-1] == 0.0, c
        # ... and (dt, df) equals the twin's for every one of them
        assert (int(got["ttweak"][i]), int(got["ftweak"][i])) == (tw["tt"], tw["ft"]), c
        if tw["metric"] > 0:
            worst_m = max(worst_m, abs(float(got["metric"][i]) - tw["metric"]) / tw["metric"])
        top = np.abs(tw["llr"]).max()
        if top > 0:
            worst_l = max(worst_l, np.abs(got["llr"][i] - tw["llr"]).max() / top)
        else:                                                               # the all-zero frame: std = 0, all-zero LLRs, the floor report
            assert not got["llr"][i].any() and (int(got["ttweak"][i]), int(got["ftweak"][i])) == (-4, -2)
        assert abs(int(got["snr"][i]) - tw["snr"]) <= 1
    print(f"ft4 demod n = {n}: metric {worst_m:.3e}, llr {worst_l:.3e}")
    assert worst_m <= METRIC_BOUND and worst_l <= LLR_BOUND
    if n >= 6:                                                              # the crafted ones decode, but for the noise and the zero frame
        ok, lo, hi, _, _, _ = handle.ft4_ldpc(got["llr"][:6], handle.cfg.bp_nc0_b, handle.cfg.bp_iters_b)
        assert list(ok) == [1, 1, 1, 1, 0, 0] and set(cases.join_words(lo[:4], hi[:4])) == {cases.DEMOD_WORD}


# ----------------------------------------------------------------------------- 8. back end on raw vectors
SIGMA = 0.5          # BPSK in noise at 6 dB: about four hard errors in 174 bits


@pytest.mark.parametrize("n", [1, 3, 130])
def test_back_end_on_raw_vectors(handle, n):
    words = cases.random_words(n, n)
    c = handle.cfg
    ft8 = cases.noisy_llrs(words, SIGMA, n, scrambled=False)
    ok8, lo8, hi8 = handle.ldpc(ft8, c.bp_nc0_b, c.bp_iters_b)[:3]
    assert ok8.mean() > 0.95 and all(w == g for w, g, k in zip(words, cases.join_words(lo8, hi8), ok8) if k)
    llr = cases.noisy_llrs(words, SIGMA, n)
    ok, lo, hi = handle.ft4_ldpc(llr, c.bp_nc0_b, c.bp_iters_b)[:3]
    assert np.array_equal(ok, ok8)                                          # the same noise on the same code: the same outcome
    assert all(w == g for w, g, k in zip(words, cases.join_words(lo, hi), ok) if k)
    oko, loo, hio, _, hd = handle.ft4_osd(llr, c.osd_single, c.osd_double, 0, 0)
    assert oko.mean() > 0.95 and all(w == g for w, g, k in zip(words, cases.join_words(loo, hio), oko) if k) and hd[oko == 1].max() <= 20
    # the FT8 entries do not descramble, the FT4 ones do: neither returns the planted word from the other's vectors
    x8 = handle.ldpc(llr, c.bp_nc0_b, c.bp_iters_b)
    x4 = handle.ft4_ldpc(ft8, c.bp_nc0_b, c.bp_iters_b)
    assert all(not k or g == w ^ ft4.RVEC for w, g, k in zip(words, cases.join_words(x8[1], x8[2]), x8[0]))
    assert all(not k or g == w ^ ft4.RVEC for w, g, k in zip(words, cases.join_words(x4[1], x4[2]), x4[0]))


def test_back_end_message_types_and_noise(handle):
    c = handle.cfg
    ext = cases.ext_words()
    words = [w for _, _, w in ext]
    llr = cases.noisy_llrs(words, 0.3, 77)
    ok, lo, hi = handle.ft4_ldpc(llr, c.bp_nc0_b, c.bp_iters_b, mask=_lib.MT_ALL)[:3]
    assert list(ok) == [1] * 6 and cases.join_words(lo, hi) == words
    assert not handle.ft4_ldpc(llr, c.bp_nc0_b, c.bp_iters_b, mask=0)[0].any()          # refused without their bits
    oko, loo, hio, _, _ = handle.ft4_osd(llr, c.osd_single, c.osd_double, 0, 0, mask=_lib.MT_ALL)
    names = [n for n, _, _ in ext]
    for k, name in enumerate(names):                                        # free text and telemetry come from BP, never from OSD
        assert bool(oko[k]) == (name not in ("free_text", "telemetry")), name
        assert not oko[k] or cases.join_words(loo[k:k + 1], hio[k:k + 1]) == [words[k]]
    assert not handle.ft4_osd(llr, c.osd_single, c.osd_double, 0, 0, mask=0)[0].any()
    for name, w in zip(names, words):                                       # one type's bit admits that type alone
        got = handle.ft4_ldpc(llr, c.bp_nc0_b, c.bp_iters_b, mask=_lib.MSG_TYPE_BITS[name])[0]
        assert [bool(g) for g in got] == [m == name for m in names]
    # 130 noise-only vectors: nothing under the default distance gate
    rng = np.random.Generator(np.random.Philox(key=130))
    noise = (ft4.LLR_SCALE * rng.standard_normal((130, 174))).astype(np.float32)
    gate = handle.ft4_info()["osd_max_hd"]
    assert gate == ft4.OSD_MAX_HD_DEFAULT
    for mask, hd in ((0, gate), (_lib.MT_ALL, ft4.OSD_MAX_HD_MSG_TYPES)):   # ... and the opt-in types' own gate (Receiver's with msg_types)
        assert not handle.ft4_ldpc(noise, c.bp_nc0_b, c.bp_iters_b, mask=mask)[0].any()
        assert not handle.ft4_osd(noise, c.osd_single, c.osd_double, 0, hd, mask=mask)[0].any()


def test_ft8_raw_entries_are_what_they_were():
    """ft8rx_ldpc / ft8rx_osd on FT8 vectors: a handle that has run FT4 returns what a fresh one returns"""
    words = cases.random_words(40, 8)
    llr = cases.noisy_llrs(words, 0.7, 8, scrambled=False)
    fresh, used = _lib.Handle(max_frames=1), _lib.Handle(max_frames=1)
    try:
        used.ft4_decode(cases.six()[0])
        used.ft4_ldpc(llr, 30, 20)
        a, b = fresh.ldpc(llr, fresh.cfg.bp_nc0_b, fresh.cfg.bp_iters_b), used.ldpc(llr, used.cfg.bp_nc0_b, used.cfg.bp_iters_b)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[0].sum() >= 20
        a, b = fresh.osd(llr, want_hd=True), used.osd(llr, want_hd=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[0].sum() >= 20
    finally:
        fresh.close(); used.close()


# ----------------------------------------------------------------------------- 9. end to end
def _texts(msgs):
    return sorted(" ".join(x for x in m["msg_tuple"] if x) for m in msgs)


@pytest.fixture(scope="module")
def rx():
    r = Receiver("", None, max_frames=3)
    yield r
    r.close()


def test_end_to_end(rx):
    frames = [cases.six(i) for i in cases.SIX]
    audio = np.stack([f[0] for f in frames])
    cs = ["240101_000000", "240101_000007.5", "240101_000015"]
    out, rec, cnt = rx.decode_frames_ft4(audio, cs, return_records=True)
    assert len(out) == 3
    for f, (x, truth) in enumerate(frames):
        assert _texts(out[f]) == sorted(t["msg"] for t in truth)
        by = {" ".join(m["msg_tuple"]): m for m in out[f]}
        for t in truth:
            m = by[t["msg"]]
            assert abs(m["tsec"] - t["t0"]) <= 0.005 and abs(m["fHz"] - t["f0"]) <= 3.0, (t, m["tsec"], m["fHz"])
            assert m["mode"] == "FT4" and " + " in m["all_txt_format"] and " ~ " not in m["all_txt_format"] and m["their_tx_cycle"] == f % 2
            assert abs(int(m["their_snr"]) - t["snr"]) <= 6 and m["cyclestart_string"] == cs[f]
        # a frame decoded alone gives the records it gives inside the batch, byte for byte
        one, rec1, cnt1 = rx.decode_frames_ft4(x, [cs[f]], return_records=True)
        assert _texts(one[0]) == _texts(out[f]) and int(cnt1[0]) == int(cnt[f])
        assert rec1[0, :int(cnt1[0])].tobytes() == rec[f, :int(cnt[f])].tobytes()
    assert rx.decode_frame_ft4(frames[0][0]) and _texts(decode_frames_ft4(audio[:1])[0]) == _texts(out[0])


def test_end_to_end_no_message_from_nothing(rx):
    out = rx.decode_frames_ft4(np.stack([cases.zero_frame(), cases.noise_frame()]))
    assert out == [[], []]


def test_end_to_end_max_cands():
    x, truth = cases.six()
    got = decode_frames_ft4(x[None], max_cands=2)[0]
    assert 1 <= len(got) <= 2 and set(_texts(got)) <= {t["msg"] for t in truth}


def test_end_to_end_message_types():
    ext = {n: (t, w) for n, t, w in cases.ext_words()}
    names = ("rtty_ru", "field_day", "eu_vhf")
    std = synth.pack77("CQ", "K1ABC", "FN42")
    x = ft4.make_frame(31, words=[ext[n][1] for n in names] + [std], snr_range=(0.0, 5.0))
    plain = decode_frames_ft4(x[None])[0]
    assert _texts(plain) == ["CQ K1ABC FN42"] and "msg_type" not in plain[0]
    full = decode_frames_ft4(x[None], msg_types="all")[0]
    want = {"rtty_ru": "TU; K1ABC W9XYZ 579 WI", "field_day": "K1ABC W9XYZ R 17B EMA"}
    got = _texts(full)
    assert len(got) == 4 and "CQ K1ABC FN42" in got and all(want[n] in got for n in want)
    assert sorted(m["msg_type"] for m in full) == ["0.4", "1", "3", "5"]
    eu = [m for m in full if m["msg_type"] == "5"][0]                       # the hashed calls are not in the frame's fresh table
    assert eu["msg_tuple"][2] == "R 590003 IO91NP"


# ----------------------------------------------------------------------------- 10. nothing else moved
def test_ft8_after_ft4_is_byte_identical_and_no_workspace_without_ft4():
    audio = synth.make_frame(7, n_signals=12, snr_range=(-12.0, 5.0))
    fresh, used = _lib.Handle(max_frames=1), _lib.Handle(max_frames=1)
    try:
        assert fresh.ft4_info()["workspace_bytes"] == 0 and used.ft4_info()["workspace_bytes"] == 0
        rec4, cnt4 = used.ft4_decode(cases.six()[0])[:2]
        assert (rec4[0, :int(cnt4[0])]["status"] == _lib.ST_DECODED).sum() >= 6
        assert used.ft4_info()["workspace_bytes"] > ft4.ROWS * ft4.COLS * 4 and fresh.ft4_info()["workspace_bytes"] == 0
        a, b = fresh.decode_batch(audio), used.decode_batch(audio)
        n, ne = int(a[1][0]), int(a[3][0])
        assert n > 0 and ne > 0 and int(b[1][0]) == n and int(b[3][0]) == ne and a[0][0, :n].tobytes() == b[0][0, :n].tobytes()
        key = lambda ev: sorted(e.tobytes() for e in ev)
        assert key(a[2][0, :ne]) == key(b[2][0, :ne])                       # the log's order is the atomics' (kernels/common.hpp)
        assert fresh.ft4_info()["workspace_bytes"] == 0                     # FT8 work allocates nothing of FT4's
    finally:
        fresh.close(); used.close()


# ----------------------------------------------------------------------------- 11. refusals
@pytest.mark.parametrize("kw, name", [(dict(my_call="K1ABC"), "my_call / dx_call"), (dict(recall=True), "recall"), (dict(weak=True), "weak=True"),
                                      (dict(reports=True), "reports=True"), (dict(float_frames=True), "float_frames=True")])
def test_refusals_by_name(kw, name):
    r = Receiver("", None, max_frames=1, **kw)
    try:
        with pytest.raises(_lib.Ft8rxError, match=r"FT4 decoding \(decode_frames_ft4\) is not supported together with " + name.replace("(", r"\(")):
            r.decode_frames_ft4(cases.zero_frame())
    finally:
        r.close()


def test_refusals_of_the_library(rx, handle):
    with pytest.raises(_lib.Ft8rxError, match=r"passes > 1"):
        rx.decode_frames_ft4(cases.zero_frame(), passes=2)
    with pytest.raises(_lib.Ft8rxError, match="90000"):
        rx.decode_frames_ft4(np.zeros(180000, np.int16))
    with pytest.raises(_lib.Ft8rxError, match="90000"):
        handle.ft4_decode(np.zeros((1, 89999), np.int16))
    with pytest.raises(_lib.Ft8rxError, match="n <= 3"):
        handle.ft4_grid(np.zeros((4, 90000), np.int16))
    with pytest.raises(_lib.Ft8rxError, match="out of range"):
        handle.ft4_demod(cases.zero_frame(), [0], [571], [0])
    with pytest.raises(_lib.Ft8rxError, match="ft8rx_ft4_set"):
        handle.ft4_set(sync_min=-1.0)
    h = _lib.Handle(max_frames=1)
    try:
        cap = _lib.packed_capacity(1)
        bufs = (h.pinned_bytes(cap), h.pinned_bytes(cap))
        h.set_packed_output(bufs[0].ctypes.data, bufs[1].ctypes.data, cap, keep=bufs)
        with pytest.raises(_lib.Ft8rxError, match=r"FT4 decoding \(ft8rx_ft4_decode_batch\) is not supported together with the packed output"):
            h.ft4_decode(cases.zero_frame())
        h.set_packed_output(None, None, 0)
        for on, off, name in ((lambda: h.set_weak(True), lambda: h.set_weak(False), "ft8rx_set_weak"),
                              (lambda: h.set_reports(True), lambda: h.set_reports(False), "ft8rx_set_reports"),
                              (lambda: h.set_ap_calls("K1ABC", None), lambda: h.set_ap_calls(None, None), "ft8rx_set_ap_calls")):
            on()
            with pytest.raises(_lib.Ft8rxError, match="not supported together with " + name):
                h.ft4_decode(cases.zero_frame())
            off()
        assert h.ft4_info()["workspace_bytes"] == 0                         # a refused call allocates nothing
        h.ft4_decode(cases.zero_frame())
    finally:
        h.close()
