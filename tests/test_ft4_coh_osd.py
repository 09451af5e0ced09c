"""FT4 OSD on the coherent LLRs without a GPU: the twin pyft8_amd/ft4.py verify_score on designed inputs and
on fixed seeds, then which calls Receiver(ft4_coh_osd=True) makes on its handle, the two refusals, and the new entry points in the
header, the prototype table and the built library."""
import os
import types

import numpy as np
import pytest

import ft4_cases as cases
from conftest import ROOT
from pyft8_amd import _abi, _lib, ft4, receiver, synth
from test_abi import c_prototypes, mismatches
from test_ft4_coherent import Recorder, take

NEW = ("ft8rx_ft4_set_coh_osd", "ft8rx_ft4_coh_osd_info", "ft8rx_ft4_verify")
OTHER_WORD = cases.random_words(1, 3)[0]          # a standard word that shares no field with DEMOD_WORD


def winner(x, f0, h0):
    d = ft4.demod(x, f0, h0)
    return d["tt"], d["ft"], ft4.coherent_llrs(x, f0, h0, d["tt"], d["ft"])["q"]


def tone_burst(x, start, fq, tone, amp=1000.0):
    """576 samples of tone `tone` of a carrier fq (x 12000 / 4608 Hz) from sample `start` on, added to x"""
    n = np.arange(ft4.NSPS)
    x[start:start + ft4.NSPS] += amp * np.cos(2 * np.pi * (fq + 8 * tone) * n / 4608.0)


# ---- 1. the twin on designed inputs
def test_clean_signal_scores_near_206_and_a_wrong_word_less_than_half():
    """The wrong word keeps the four all-sync runs and the symbols it shares by chance: 40 random standard words score 0.32 .. 0.53 of
    the right one's, two of them above half -- a word that shares a call with the planted one sits at the top of that range"""
    x = ft4.frame_with_signals(1, [(cases.DEMOD_WORD, 1000.0, 0.504, 0.0)], noise=False)
    tt, ft, q = winner(x, 96, 42)
    assert (tt, ft, q) == (0, 0, 0)
    own = ft4.verify_score(x, 96, 42, tt, ft, q, cases.DEMOD_WORD)
    other = ft4.verify_score(x, 96, 42, tt, ft, q, OTHER_WORD)
    print(f"ft4 verify twin, noise-free signal: own word {own:.2f}, another standard word {other:.2f}")
    assert abs(own - 206.0) <= 0.02 * 206.0 and other < 0.5 * own


@pytest.mark.parametrize("q", [-4, 4])
def test_residual_of_four_quarter_steps(q):
    """A noise-free signal one fine step (2.6042 Hz = four quarter steps) off the candidate's frequency, the fine tweak held at 0: q = +-4
    takes the whole residual and the score is the clean one up to the loss inside a symbol; the opposite q turns every run against
    itself"""
    x = ft4.frame_with_signals(1, [(cases.DEMOD_WORD, 1000.0 + q * ft4.DF_HZ / 4, 0.504, 0.0)], noise=False)
    s = {k: ft4.verify_score(x, 96, 42, 0, 0, k, cases.DEMOD_WORD) for k in (-4, 0, 4)}
    assert s[q] > 0.95 * 206.0 and s[0] < 0.7 * s[q] and s[-q] < 0.1 * s[q], s


@pytest.mark.parametrize("q", [-4, 0, 4])
def test_energy_in_the_outer_symbols_alone_scores_zero(q):
    x = np.zeros(ft4.NFRAME)
    start = ft4.HOP * 10
    tone_burst(x, start, 4 * 96, 0)
    tone_burst(x, start + 104 * ft4.NSPS, 4 * 96, 0)
    assert np.abs(ft4.complex_amplitudes(x, 96, 10, 0, 0)[[0, 104]]).min(axis=0).max() > 1e5      # the energy is there ...
    assert ft4.verify_score(x, 96, 10, 0, 0, q, cases.DEMOD_WORD) == 0.0                          # ... and never enters


@pytest.mark.parametrize("q", [-4, 0, 4])
def test_the_last_run_has_three_symbols(q):
    """Energy in symbols 101 .. 103 alone: A is the one three-term sum, N their power"""
    x = np.zeros(ft4.NFRAME)
    start, T = ft4.HOP * 10, ft4.tones105(cases.DEMOD_WORD)
    for s in (101, 102, 103):
        tone_burst(x, start + s * ft4.NSPS, 4 * 96, T[s], amp=500.0 + s)
    tone_burst(x, start + 104 * ft4.NSPS, 4 * 96, 0)                                               # symbol 104: left out
    C = ft4.complex_amplitudes(x, 96, 10, 0, 0) * np.exp(-2j * np.pi * ((q * np.arange(105)) % 32) / 32.0)[:, None]
    direct = abs(C[101][T[101]] + C[102][T[102]] + C[103][T[103]]) / np.sqrt((np.abs(C[101:104]) ** 2).sum() / 412.0)
    got = ft4.verify_score(x, 96, 10, 0, 0, q, cases.DEMOD_WORD)
    assert direct > 10.0 and abs(got - direct) <= 1e-12 * direct


def test_edges():
    audio, cands = cases.demod_frames()
    for q in (-4, 0, 4):
        assert ft4.verify_score(cases.zero_frame(), 200, 30, -4, -2, q, cases.DEMOD_WORD) == 0.0
    for k, what in ((0, "starts before the frame"), (1, "runs past the frame")):
        f, f0, h0, name = cands[k]
        assert name == what
        tt, ft, q = winner(audio[f], f0, h0)
        s = ft4.verify_score(audio[f], f0, h0, tt, ft, q, cases.DEMOD_WORD)
        assert np.isfinite(s) and 150.0 < s < 206.0, (what, s)
        for other in (-4, 4):                                                      # a residual the signal does not have turns the symbols of a
            t = ft4.verify_score(audio[f], f0, h0, tt, ft, other, cases.DEMOD_WORD)    # run against each other: finite, and it can only lose
            assert q not in (-4, 4) and np.isfinite(t) and 0.0 < t < s, (what, other, t)


# ---- 2. separation on fixed seeds
@pytest.fixture(scope="module")
def separation():
    """30 truths at -17 dB (frames 7000 .. 7002) at their rounded positions, and 60 noise candidates (frames 9100 .. 9103), each at the
    winner of ft4.demod and the q of ft4.coherent_llrs -> (scores of the true words, of random standard words on the same candidates,
    of random standard words on noise)"""
    wrong = cases.random_words(64, 11)
    true, other, noise = [], [], []
    for i in range(3):
        x, truth = ft4.make_frame(7000 + i, n_signals=10, snr_range=(-17, -17), min_sep_hz=150, return_truth=True)
        for t in truth:
            f0, h0 = round(t["f0"] / ft4.BIN_HZ), round(t["t0"] * 12000 / 144)
            tt, ft, q = winner(x, f0, h0)
            true.append(ft4.verify_score(x, f0, h0, tt, ft, q, t["word"]))
            other.append(ft4.verify_score(x, f0, h0, tt, ft, q, wrong[len(other)]))
    for i in range(4):
        x = ft4.make_frame(9100 + i, n_signals=0)
        for j in range(15):
            f0, h0 = 20 + 35 * j + 3 * i, -30 + 12 * j
            noise.append(ft4.verify_score(x, f0, h0, *winner(x, f0, h0), wrong[(15 * i + j) % 64]))
    return np.sort(true), np.sort(other), np.sort(noise)


def test_separation_on_fixed_seeds(separation):
    """These numbers bound the float64 twin on these seeds alone -- no kernel, no default.  Measured: the 18 synchronised truths score
    105.8 .. 130.2 (the other 12, which ft4.demod did not synchronise, 43.8 .. 88.9), a random standard word on the same candidates
    42.9 .. 81.1 (the four Costas blocks are the signal's whatever the word says), on noise 36.3 .. 54.6 (26 sqrt(pi) / 2 sqrt(4) = 46
    is the mean of 26 Rayleigh terms)."""
    true, other, noise = separation
    print(f"ft4 verify twin at -17 dB: truths {true.round(1)}, another word {other.min():.1f} .. {other.max():.1f}, noise {noise.min():.1f} .. {noise.max():.1f}")
    sync = true[true >= 105.0]
    assert len(sync) == 18 and sync.max() <= 131.0 and true[true < 105.0].max() <= 89.0
    assert other.max() <= 82.0 and noise.max() <= 55.0 and noise.min() >= 36.0
    assert sync.min() - max(other.max(), noise.max()) >= 24.0                     # the gap a gate has to sit in


# ---- 3. host traces, refusals
def test_host_traces(monkeypatch):
    monkeypatch.setattr(Recorder, "ft4_set_coh_osd", lambda self, on, min_score=None, max_hd=None: Recorder.calls.append(f"ft4_set_coh_osd({on}, {min_score})"),
                        raising=False)
    monkeypatch.setattr(_lib, "Handle", Recorder)
    take()
    x = np.zeros((2, _lib.FT4_NSAMP), np.int16)
    wide = types.SimpleNamespace(channels={"FT4": [0, 1]}, bands=None, n_channels=2, seen=[{}, {}])
    on = receiver.Receiver("", None, autostart=False, max_frames=2, ft4_coherent=True, ft4_coh_osd=True, ft4_coh_osd_min_score=101.5)
    assert on.ft4_coh_osd is True and on.decode_frames_ft4(x) == [[], []]
    assert take() == ["ft4_set", "ft4_set_coherent(True)", "ft4_set_coh_osd(True, 101.5)", "ft4_set_range", "ft4_decode(2)"]      # once per _ft4_set
    on._live_pass_ft4(wide, 0, 0, _lib.FT4_NSAMP, [])
    assert take() == ["ft4_set", "ft4_set_coherent(True)", "ft4_set_coh_osd(True, 101.5)", "ft4_set_range", f"ddc_stream_frames({_lib.FT4_NSAMP})",
                      "ft4_enqueue(2)", "fetch(2)"]
    for kw, ms in (({}, None), ({"msg_types": "all"}, ft4.COH_OSD_MIN_SCORE_MSG_TYPES), ({"msg_types": "all", "ft4_coh_osd_min_score": 90.0}, 90.0)):
        rx = receiver.Receiver("", None, autostart=False, max_frames=2, ft4_coherent=True, ft4_coh_osd=True, **kw)
        rx.decode_frames_ft4(x)
        assert f"ft4_set_coh_osd(True, {ms})" in take(), kw                        # the library's default, or the opt-in types' own gate
    for kw in ({}, {"ft4_coh_osd": False}):                                        # never without the keyword
        off = receiver.Receiver("", None, autostart=False, max_frames=2, ft4_coherent=True, **kw)
        assert off.ft4_coh_osd is False and off.decode_frames_ft4(x) == [[], []]
        assert take() == ["ft4_set", "ft4_set_coherent(True)", "ft4_set_range", "ft4_decode(2)"]


def test_refusals_by_name():
    for bad in (1, 0, "yes", None):
        with pytest.raises(_lib.Ft8rxError, match="ft4_coh_osd must be True or False"):
            receiver.Receiver("", None, autostart=False, ft4_coherent=True, ft4_coh_osd=bad)
    for kw in ({}, {"ft4_coherent": False}):
        with pytest.raises(_lib.Ft8rxError, match="ft4_coh_osd=True needs ft4_coherent=True"):
            receiver.Receiver("", None, autostart=False, ft4_coh_osd=True, **kw)


# ---- 4. the ABI
def test_header_and_prototype_table():
    text = open(os.path.join(ROOT, "include", "ft8rx.h")).read()
    header = c_prototypes(text, r"ft8rx_ft4_(?:set_coh_osd|coh_osd_info|verify)")
    assert sorted(header) == sorted(NEW)
    assert mismatches({n: _abi.PROTOTYPES[n] for n in NEW}, header) == []
    assert [len(_abi.PROTOTYPES[n][1]) for n in NEW] == [4, 5, 14]
    assert all(text.count(n) >= 2 for n in NEW)                                   # the map of the ABI and the declaration
    for name, value in (("FT8RX_FT4_COH_OSD_MIN_SCORE_DEFAULT", f"{ft4.COH_OSD_MIN_SCORE_DEFAULT}f"), ("FT8RX_FT4_COH_OSD_MAX_HD_DEFAULT", str(ft4.COH_OSD_MAX_HD_DEFAULT))):
        assert any(line.split()[:3] == ["#define", name, value] for line in text.splitlines()), name


def test_built_library_exports_the_symbols():
    for wide in (False, True):
        for n in NEW:
            assert getattr(_lib.lib(wide), n).argtypes == list(_abi.PROTOTYPES[n][1])
    assert callable(_lib.Handle.ft4_set_coh_osd) and callable(_lib.Handle.ft4_verify) and callable(_lib.Handle.ft4_coh_osd_info)
