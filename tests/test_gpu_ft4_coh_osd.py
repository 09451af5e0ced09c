"""FT4 OSD on the coherent LLRs behind a whole-message score, on the GPU (k_ft4_verify and the opt-in step of
the FT4 chain): the stage against the float64 twin ft4.verify_score, its tones against the host encoder, the setting off = the chain as
it was, on with designed, strong and weak signals, and with the other knobs.  Run with -m gpu on an MI355X.

The stage's bound is not this kernel's own error: it is the parent's asserted bound of the 576-sample sums (AMP_BOUND = 6e-7 of a row's
norm, tests/test_gpu_ft4.py; a row of 576 samples x has the norm 24 ||x||_2, as tests/ft4_weak_cases.py takes it), carried through the
score's definition (score_bound below)."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import ft4_cases as cases
from pyft8_amd import _lib, ft4, messages, synth
from pyft8_amd.receiver import Receiver, decode_frames_ft4
from test_gpu_ft4 import AMP_BOUND
from test_gpu_ft4_coherent import _same, _texts
from test_gpu_ft4_weak import weak_frames

pytestmark = pytest.mark.gpu


def score_bound(x, f0, h0, tt, ft, q, word):
    """-> (the twin's score, the bound of |kernel - twin| that follows from AMP_BOUND).  Every C[s][t] is off by at most
    d_s = AMP_BOUND x 24 ||x_s||_2 (x_s: the symbol's 576 samples, zeros outside the frame; a turn by an exact table entry keeps it).
    With nrm = sqrt(sum over symbols 1 .. 103 and the 4 tones of |C|^2), score = sqrt(412) A / nrm:  |dA| <= D1 = the sum of d_s over
    symbols 1 .. 103 (a run adds at most four values, a magnitude is 1-Lipschitz), |d nrm| <= D2 = sqrt(4 sum d_s^2) (the norm of the
    412 errors), hence |d score| <= (sqrt(412) D1 + score D2) / (nrm - D2); plus the rounding of the stored float32.  On digital
    silence nrm = D2 = 0 and the score is exactly 0."""
    x = np.asarray(x, np.float64)
    C = ft4.complex_amplitudes(x, f0, h0, tt, ft) * np.exp(-2j * np.pi * ((int(q) * np.arange(ft4.NSYM)) % 32) / 32.0)[:, None]
    A, N = ft4.verify_terms(C, ft4.tones105(word))
    nrm = np.sqrt(412.0 * N)
    if nrm == 0.0:
        return 0.0, 0.0
    score = np.sqrt(412.0) * A / nrm
    d = AMP_BOUND * 24.0 * np.sqrt((ft4._symbols(x, ft4.HOP * h0 + ft4.DT_STEP * tt + ft4.NSPS * np.arange(1, ft4.NSYM - 1)) ** 2).sum(axis=1))
    D1, D2 = d.sum(), np.sqrt(4.0 * (d * d).sum())
    assert nrm > D2
    return score, (np.sqrt(412.0) * D1 + score * D2) / (nrm - D2) + score * 2.0 ** -23


# ----------------------------------------------------------------------------- 1. the stage against the twin
@functools.lru_cache(maxsize=None)
def stage_cases():
    """the 65 crafted candidates of the coherent test at the twin's winners and residuals, each with its planted word and a wrong word
    -> (audio, candidates, winners (tt, ft, q), [(twin score, bound)] for the planted word, the same for the wrong word)"""
    audio, cands = cases.demod_candidates(65)
    wrong = cases.random_words(65, 23)
    win, own, other = [], [], []
    for i, c in enumerate(cands):
        t = cases.twin_demod(*c)
        q = ft4.coherent_llrs(audio[c[0]], c[1], c[2], t["tt"], t["ft"])["q"]
        win.append((t["tt"], t["ft"], q))
        own.append(score_bound(audio[c[0]], c[1], c[2], t["tt"], t["ft"], q, cases.DEMOD_WORD))
        other.append(score_bound(audio[c[0]], c[1], c[2], t["tt"], t["ft"], q, wrong[i]))
    return audio, cands, win, own, other, wrong


@pytest.mark.parametrize("n", [1, 65])
def test_stage_against_the_twin(n):
    audio, cands, win, own, other, wrong = stage_cases()
    h = _lib.Handle(max_frames=3)
    try:
        col = lambda k: [c[k] for c in cands[:n]]
        args = (col(0), col(1), col(2), [w[0] for w in win[:n]], [w[1] for w in win[:n]], [w[2] for w in win[:n]])
        got_own = h.ft4_verify(audio, *args, [cases.DEMOD_WORD] * n)
        got_other = h.ft4_verify(audio, *args, wrong[:n])
        assert h.ft4_coh_osd_info()["workspace_bytes"] == 0 and h.ft4_coh_info()["workspace_bytes"] == 0      # the stage entry owns nothing of the chain's
    finally:
        h.close()
    worst = 0.0
    for i in range(n):
        for got, (ref, bound) in ((got_own[i], own[i]), (got_other[i], other[i])):
            if ref == 0.0:                                                      # the all-zero frame: exactly the twin
                assert cands[i][0] == 2 and got == 0.0
                continue
            assert np.isfinite(got) and abs(float(got) - ref) <= bound, (cands[i], float(got), ref, bound)
            worst = max(worst, abs(float(got) - ref) / bound)
    print(f"ft4 verify stage, n = {n}: worst share of the bound {worst:.3f}; scores of the planted word {min(float(g) for g in got_own):.1f} .. "
          f"{max(float(g) for g in got_own):.1f}")
    if n == 65:
        assert sum(c[0] == 2 for c in cands) >= 1 and sum(c[0] == 1 for c in cands) >= 1          # the all-zero and the noise candidate took part
        assert min(float(got_own[i]) for i in range(4)) > 150.0 > max(float(g) for g in got_other)      # the four planted signals at their own positions


def test_tones_are_the_host_encoder_s():
    """the kernel's own encoder (rvec, CRC-14, the 83 parity bits, Gray map, Costas blocks) against ft8rx_ft4_encode_tones, byte for byte"""
    words = cases.random_words(50, 5) + [w for _, _, w in cases.ext_words()] + [0, 2 ** 77 - 1]
    n = len(words)
    audio = cases.demod_frames()[0]
    h = _lib.Handle(max_frames=3)
    try:
        sc, tones = h.ft4_verify(audio, [0] * n, [96] * n, [-25] * n, [0] * n, [0] * n, [0] * n, words, want_tones=True)
    finally:
        h.close()
    want = _lib.ft4_encode_tones(*cases.split_words(words))
    assert tones.shape == (n, 105) and tones.tobytes() == np.asarray(want, np.uint8).tobytes() and np.isfinite(sc).all()
    assert [list(t) for t in tones[:3]] == [ft4.tones105(w) for w in words[:3]]


# ----------------------------------------------------------------------------- 2. off is the chain as it was
def test_off_is_the_parent():
    six = np.stack([cases.six(i)[0] for i in cases.SIX])
    crafted = cases.demod_frames()[0]
    weak = weak_frames()[0][:3]
    ft8 = synth.make_frame(7, n_signals=12, snr_range=(-12.0, 5.0))
    never, toggled, fresh = _lib.Handle(max_frames=3), _lib.Handle(max_frames=3), _lib.Handle(max_frames=3)
    try:
        never.ft4_set_coherent(True)
        a = [never.ft4_decode(x) for x in (six, crafted, weak)]
        figures = lambda h: (h.ft4_info()["workspace_bytes"], h.ft4_coh_info(), h.ft4_weak_info())
        base = figures(never)
        off = dict(workspace_bytes=0, on=False, min_score=float(np.float32(ft4.COH_OSD_MIN_SCORE_DEFAULT)), max_hd=ft4.COH_OSD_MAX_HD_DEFAULT)
        assert never.ft4_coh_osd_info() == off
        toggled.ft4_set_coh_osd(True)
        toggled.ft4_decode(crafted)                                             # without the coherent step the setting does nothing
        assert toggled.ft4_coh_osd_info() == dict(off, on=True)
        toggled.ft4_set_coherent(True)
        toggled.ft4_decode(weak)
        info = toggled.ft4_coh_osd_info()
        S = 3 << 8
        assert info["on"] and info["workspace_bytes"] == 4 * S + 2 * S * 174 * 4 + 2 * S * 24 + 4 * (2 * S + 1) + 4 * 2 * S
        assert figures(toggled) == base                                         # the three other figures keep theirs
        toggled.ft4_set_coh_osd(True, 123.5, 50)
        assert toggled.ft4_coh_osd_info() == dict(workspace_bytes=info["workspace_bytes"], on=True, min_score=123.5, max_hd=50)
        toggled.ft4_set_coh_osd(False)
        assert toggled.ft4_coh_osd_info() == dict(off, workspace_bytes=info["workspace_bytes"])
        fresh.ft4_set_coherent(True)
        for x, want in zip((six, crafted, weak), a):
            _same(toggled.ft4_decode(x), want)
            _same(fresh.ft4_decode(x), want)
        assert fresh.ft4_coh_osd_info() == off and never.ft4_coh_osd_info() == off
        # FT8 behind an FT4 batch that ran the step
        toggled.ft4_set_coh_osd(True)
        toggled.ft4_decode(weak)
        clean = _lib.Handle(max_frames=3)
        try:
            _same(toggled.decode_batch(ft8), clean.decode_batch(ft8))
        finally:
            clean.close()
    finally:
        never.close(); toggled.close(); fresh.close()


# ----------------------------------------------------------------------------- 3. on, designed: only the new step can decode these
DESIGNED = (175004, 175006)           # make_frame indices: six signals at -13 dB each, every one with hard errors in all three LLR sets


@functools.lru_cache(maxsize=None)
def designed_frames():
    fr = [ft4.make_frame(i, n_signals=6, snr_range=(-13.0, -13.0), min_sep_hz=150, return_truth=True) for i in DESIGNED]
    return np.stack([f[0] for f in fr]), [sorted(t["msg"] for t in f[1]) for f in fr]


def _frame_texts(res, f):
    return sorted(" ".join(x for x in m["msg_tuple"] if x) for m in messages.package_frame(res[0][f], int(res[1][f]), res[2][f], int(res[3][f])))


def test_on_designed_signals():
    """BP can take a vector only if it has no hard error (bp_nc0_b = 0, one iteration), the single-symbol OSD only within distance 1:
    with the setting off nothing decodes; with it on, OSD on the coherent rows takes every planted signal"""
    audio, planted = designed_frames()
    cfg = _lib.default_config(bp_nc0_a=0, bp_iters_a=1, bp_nc0_b=0, bp_iters_b=1)
    h = _lib.Handle(cfg, max_frames=2)
    try:
        h.ft4_set(0, 1)
        h.ft4_set_coherent(True)
        off = h.ft4_decode(audio)
        assert [_frame_texts(off, f) for f in range(2)] == [[], []]
        assert not (off[0]["status"] == _lib.ST_DECODED).any() and not off[3].any()
        h.ft4_set_coh_osd(True)
        on = h.ft4_decode(audio)
        assert [_frame_texts(on, f) for f in range(2)] == planted
        for f in range(2):
            r = on[0][f, :int(on[1][f])]
            dec = r[r["status"] == _lib.ST_DECODED]
            assert len(dec) == 6 and int(on[3][f]) == 6
            assert (dec["ipass"] == 5).all() and (dec["method"] == _lib.M_OSD).all() and not dec["ap"].any() and np.isin(dec["nsync"], (2, 4)).all()
            ev = on[2][f, :6]
            assert (ev["ipass"] == 5).all() and sorted(ev["slot"]) == sorted(np.where(dec["nsync"] == 2, 1, 2))
            for x in dec:
                word = (int(x["msg_hi"]) << 64) | int(x["msg_lo"])
                pos = (int(x["f0_idx"]), int(x["h0_idx"]), int(x["ttweak"]), int(x["ftweak"]))
                c = ft4.coherent_llrs(audio[f], *pos)
                bits = cases.codeword_bits(word) > 0.5
                errs = [int(((c[k] > 0) != bits).sum()) for k in ("llr1", "llr2", "llr4")]
                assert errs[0] >= 2 and errs[1] >= 1 and errs[2] >= 1, (f, pos, errs)          # neither BP nor the closed gate could take it
                assert int(x["osd_hd"]) == errs[1 if x["nsync"] == 2 else 2]
                ref, bound = score_bound(audio[f], *pos, c["q"], word)
                assert ref >= ft4.COH_OSD_MIN_SCORE_DEFAULT and abs(int(x["pad2"]) / 100.0 - ref) <= bound + 0.005, (f, pos, int(x["pad2"]), ref, bound)
            rest = r[r["status"] != _lib.ST_DECODED]
            assert (rest["status"] == _lib.ST_EXHAUSTED).all() and not rest["nsync"].any() and not rest["pad2"].any()
            one = h.ft4_decode(audio[f])                                        # a frame alone: its records in the batch, byte for byte
            assert int(one[1][0]) == int(on[1][f]) and one[0][0, :int(one[1][0])].tobytes() == r.tobytes()
    finally:
        h.close()


# ----------------------------------------------------------------------------- 4. on, strong signals with the default ladder
def test_on_strong_signals_changes_nothing():
    six = np.stack([cases.six(i)[0] for i in cases.SIX])
    quiet = np.stack([cases.noise_frame(), cases.zero_frame()])
    off, on = _lib.Handle(max_frames=3), _lib.Handle(max_frames=3)
    try:
        off.ft4_set_coherent(True)
        on.ft4_set_coherent(True); on.ft4_set_coh_osd(True)
        for x in (six, quiet):
            _same(off.ft4_decode(x), on.ft4_decode(x))
        assert on.ft4_coh_osd_info()["workspace_bytes"] > 0                       # the step ran: the noise candidates went through it
    finally:
        off.close(); on.close()


# ----------------------------------------------------------------------------- 5. on, weak signals
def test_on_weak_signals():
    audio, planted = weak_frames()
    kw = dict(max_frames=8, ft4_coherent=True, ft4_weak=True)
    rx_off, rx_on = Receiver("", None, **kw), Receiver("", None, ft4_coh_osd=True, **kw)
    try:
        off = rx_off.decode_frames_ft4(audio)
        on, rec, cnt = rx_on.decode_frames_ft4(audio, return_records=True)
        n_off, n_on = sum(len(x) for x in off), sum(len(x) for x in on)
        by = [sum(d["nsym"] == k for f in on for d in f) for k in (1, 2, 4)]
        new = sum(int(((rec[f, :int(cnt[f])]["ipass"] == 5) & (rec[f, :int(cnt[f])]["nsync"] != 0) & (rec[f, :int(cnt[f])]["status"] == _lib.ST_DECODED)).sum())
                  for f in range(8))
        print(f"ft4 OSD on the coherent rows, 8 frames of 10 signals at -16.5 dB, weak search and coherent LLRs on: {n_off} messages off, {n_on} on "
              f"(nsym 1 / 2 / 4: {by}; records of the new step: {new})")
        for f in range(8):
            assert set(_texts(off[f])) <= set(_texts(on[f])), f                # a superset of the messages without the step
            assert set(_texts(on[f])) <= planted[f], f                         # and every one a planted text
            assert all(d["nsym"] in (1, 2, 4) for d in on[f])
    finally:
        rx_off.close(); rx_on.close()


# ----------------------------------------------------------------------------- 6. with the other knobs
@pytest.mark.parametrize("kw", [dict(ft4_passes=2), dict(max_cands=2), dict(ft4_reports=True)])
def test_on_with_the_other_knobs(kw):
    audio, planted = weak_frames()
    audio, planted = audio[:3], planted[:3]
    base = decode_frames_ft4(audio, ft4_coherent=True, **kw)
    got = decode_frames_ft4(audio, ft4_coherent=True, ft4_coh_osd=True, **kw)
    for f in range(3):
        assert set(_texts(got[f])) <= planted[f] and set(_texts(base[f])) <= set(_texts(got[f])), f
        assert all(d["nsym"] in (1, 2, 4) for d in got[f])
        if "ft4_reports" in kw:
            assert all("report" in d for d in got[f])
    if "max_cands" in kw:
        assert all(len(g) <= 2 for g in got)


def test_on_with_all_message_types():
    ext = {n: (t, w) for n, t, w in cases.ext_words()}
    names = ("rtty_ru", "field_day", "eu_vhf")
    std = synth.pack77("CQ", "K1ABC", "FN42")
    x = ft4.make_frame(31, words=[ext[n][1] for n in names] + [std], snr_range=(0.0, 5.0))
    base = decode_frames_ft4(x[None], msg_types="all", ft4_coherent=True)[0]
    got = decode_frames_ft4(x[None], msg_types="all", ft4_coherent=True, ft4_coh_osd=True)[0]
    assert _texts(got) == _texts(base) and len(got) == 4
    weak = weak_frames()
    got = decode_frames_ft4(weak[0][:2], msg_types="all", ft4_coherent=True, ft4_coh_osd=True)
    for f in range(2):
        assert set(_texts(got[f])) <= weak[1][f], f                                # no word of an opt-in type out of noise or a weak signal
