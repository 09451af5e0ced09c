"""FT4 coherent LLRs without a GPU: the twin pyft8_amd/ft4.py coherent_llrs -- its L = 1 path against the
demodulator's LLRs, designed residual frequencies, the edges, the gain on fixed seeds -- then which calls Receiver(ft4_coherent=True)
makes on its handle, and the new entry points in the header, the prototype table and the built library."""
import os
import types

import numpy as np
import pytest

import ft4_cases as cases
from conftest import ROOT
from pyft8_amd import _abi, _lib, ft4, receiver, synth
from test_abi import c_prototypes, mismatches

NEW = ("ft8rx_ft4_set_coherent", "ft8rx_ft4_coh_info", "ft8rx_ft4_coherent")


def hard_errors(llr, word):
    return int(((np.asarray(llr) > 0) != (cases.codeword_bits(word) > 0.5)).sum())


# ---- 1. the twin
def test_runs_of_one_are_the_demodulator():
    audio, cands = cases.demod_frames()
    for f, f0, h0, what in cands:
        d = ft4.demod(audio[f], f0, h0)
        c = ft4.coherent_llrs(audio[f], f0, h0, d["tt"], d["ft"])
        assert np.abs(c["llr1"] - d["llr"]).max() <= 1e-12, what
        assert np.abs(np.abs(ft4.complex_amplitudes(audio[f], f0, h0, d["tt"], d["ft"])) - d["amps"]).max() <= 1e-9 * max(1.0, d["amps"].max()), what
        assert c["metrics"].shape == (9,) and c["q"] in ft4.COH_Q and c["llr2"].shape == c["llr4"].shape == (174,)


def test_designed_residuals():
    """A noise-free signal 0, +-0.651, +-1.302 Hz off the fine grid: the fine sync takes the nearest 2.6042-Hz step, q the rest, in
    quarter steps -- and all three LLR sets are error-free"""
    want = {-1.302: (0, -1, 2), -0.651: (0, 0, -1), 0.0: (0, 0, 0), 0.651: (0, 0, 1), 1.302: (0, 0, 2)}
    for off, (tt, ft, q) in want.items():
        x = ft4.frame_with_signals(1, [(cases.DEMOD_WORD, 1000.0 + off, 0.504, 0.0)], noise=False)
        d = ft4.demod(x, 96, 42)
        c = ft4.coherent_llrs(x, 96, 42, d["tt"], d["ft"])
        assert (d["tt"], d["ft"], c["q"]) == (tt, ft, q), off
        m = np.sort(c["metrics"])
        assert m[-1] - m[-2] > 0.01 * m[-1], off                               # the decision is not a near-tie
        assert [hard_errors(c[k], cases.DEMOD_WORD) for k in ("llr1", "llr2", "llr4")] == [0, 0, 0], off


def test_edges():
    audio, cands = cases.demod_frames()
    z = ft4.coherent_llrs(cases.zero_frame(), 200, 30, -4, -2)
    assert z["q"] == -4 and not z["metrics"].any() and not z["llr1"].any() and not z["llr2"].any() and not z["llr4"].any()
    f, f0, h0, what = cands[0]
    assert what == "starts before the frame"
    d = ft4.demod(audio[f], f0, h0)
    c = ft4.coherent_llrs(audio[f], f0, h0, d["tt"], d["ft"])
    for k in ("llr1", "llr2", "llr4"):
        assert c[k].any() and not (c[k] == 0.0).any(), k


@pytest.fixture(scope="module")
def gain():
    """10 frames of 10 signals at -16 dB, every truth taken as the candidate -> (decodes per LLR set, decodes of any, wrong words)"""
    per, any_, wrong = [0, 0, 0], 0, 0
    for i in range(10):
        x, truth = ft4.make_frame(160000 + i, n_signals=10, snr_range=(-16, -16), min_sep_hz=150, return_truth=True)
        rows = [[], [], []]
        for t in truth:
            f0, h0 = round(t["f0"] / ft4.BIN_HZ), round(t["t0"] * 12000 / 144)
            d = ft4.demod(x, f0, h0)
            c = ft4.coherent_llrs(x, f0, h0, d["tt"], d["ft"])
            rows[0].append(d["llr"]); rows[1].append(c["llr2"]); rows[2].append(c["llr4"])
        words = [ft4.bp_decode_many(r) for r in rows]
        for k, t in enumerate(truth):
            got = [w[k] for w in words]
            for j in range(3):
                per[j] += got[j] is not None
                wrong += got[j] is not None and got[j] != t["word"]
            any_ += any(g is not None for g in got)
    return per, any_, wrong


def test_gain_on_fixed_seeds(gain):
    per, any_, wrong = gain
    print(f"ft4 coherent twin at -16 dB: runs of 1 / 2 / 4 decode {per} of 100, any of the three {any_}, wrong words {wrong}")
    assert per[0] <= 10 and any_ >= 30 and wrong == 0


# ---- 2. host traces: the setter is called once per _ft4_set, and never without the keyword
class Recorder:
    """A stand-in handle that records the FT4 calls and hands out empty results"""
    calls = []

    def __init__(self, cfg=None, device=0, max_frames=1):
        self.cfg, self.max_frames = cfg, int(max_frames)

    def set_ladder_mode(self, mode):
        pass

    def close(self):
        pass

    def _empty(self, B):
        mc = self.cfg.max_cands
        return (np.zeros((B, mc), _lib.RECORD_DTYPE), np.zeros(B, np.int32), np.zeros((B, _lib.EVENT_CAP), _lib.EVENT_DTYPE), np.zeros(B, np.int32))

    def ft4_set(self, sync_min=None, osd_max_hd=None):
        Recorder.calls.append("ft4_set")

    def ft4_set_range(self, *a):
        Recorder.calls.append("ft4_set_range")

    def ft4_set_coherent(self, on):
        Recorder.calls.append(f"ft4_set_coherent({on})")

    def ft4_decode(self, audio):
        Recorder.calls.append(f"ft4_decode({len(audio)})")
        return self._empty(len(audio))

    def ft4_staging_ptr(self):
        return 0x5A5A00

    def ddc_stream_frames(self, m_first, n_have, frame_len, ch):
        Recorder.calls.append(f"ddc_stream_frames({n_have})")

    def ft4_enqueue(self, ptr, B):
        Recorder.calls.append(f"ft4_enqueue({B})")

    def fetch(self, B):
        Recorder.calls.append(f"fetch({B})")
        return self._empty(B)


def take():
    c, Recorder.calls = Recorder.calls, []
    return c


def test_host_traces(monkeypatch):
    monkeypatch.setattr(_lib, "Handle", Recorder)
    take()
    x = np.zeros((2, _lib.FT4_NSAMP), np.int16)
    wide = types.SimpleNamespace(channels={"FT4": [0, 1]}, bands=None, n_channels=2, seen=[{}, {}])
    on = receiver.Receiver("", None, autostart=False, max_frames=2, ft4_coherent=True)
    assert on.ft4_coherent is True and on.decode_frames_ft4(x) == [[], []]
    assert take() == ["ft4_set", "ft4_set_coherent(True)", "ft4_set_range", "ft4_decode(2)"]          # before the first pass, once
    for n_have in (72000, _lib.FT4_NSAMP):                                        # the early live pass and the complete one
        out = []
        on._live_pass_ft4(wide, 0, 0, n_have, out)
        assert out == [] and take() == ["ft4_set", "ft4_set_coherent(True)", "ft4_set_range", f"ddc_stream_frames({n_have})", "ft4_enqueue(2)", "fetch(2)"]
    for kw in ({}, {"ft4_coherent": False}):
        off = receiver.Receiver("", None, autostart=False, max_frames=2, **kw)
        assert off.ft4_coherent is False and off.decode_frames_ft4(x) == [[], []]
        off._live_pass_ft4(wide, 0, 0, _lib.FT4_NSAMP, [])
        assert take() == ["ft4_set", "ft4_set_range", "ft4_decode(2)", "ft4_set", "ft4_set_range", f"ddc_stream_frames({_lib.FT4_NSAMP})", "ft4_enqueue(2)", "fetch(2)"]
    for bad in (1, 0, "yes", None):
        with pytest.raises(_lib.Ft8rxError, match="ft4_coherent must be True or False"):
            receiver.Receiver("", None, autostart=False, ft4_coherent=bad)


def test_message_dicts_say_nsym_only_when_asked():
    rows = np.zeros(2, _lib.MESSAGE_DTYPE)
    rows["f"] = [[b"CQ", b"K1ABC", b"FN42"], [b"CQ", b"W9XYZ", b"EN37"]]
    assert all("nsym" not in d for d in ft4.message_dicts(rows, 2))
    assert [d["nsym"] for d in ft4.message_dicts(rows, 2, nsym=[1, 4])] == [1, 4]
    rx = types.SimpleNamespace(ft4_coherent=True)
    rec = np.zeros((1, 8), _lib.RECORD_DTYPE)
    rec["nsync"][0, [3, 5]] = (2, 0)
    rows["cand"] = (3, 5)
    assert receiver.Receiver._ft4_nsym(rx, rec, [rows], [2], 0) == [2, 1]
    rx.ft4_coherent = False
    assert receiver.Receiver._ft4_nsym(rx, rec, [rows], [2], 0) is None


# ---- 3. the ABI
def test_header_and_prototype_table():
    text = open(os.path.join(ROOT, "include", "ft8rx.h")).read()
    header = c_prototypes(text, r"ft8rx_ft4_(?:set_coherent|coh_info|coherent)")
    assert sorted(header) == sorted(NEW)
    assert mismatches({n: _abi.PROTOTYPES[n] for n in NEW}, header) == []
    assert [len(_abi.PROTOTYPES[n][1]) for n in NEW] == [2, 3, 13]
    assert all(text.count(n) >= 2 for n in NEW)                                   # the map of the ABI and the declaration


def test_built_library_exports_the_symbols():
    for wide in (False, True):
        for n in NEW:
            assert getattr(_lib.lib(wide), n).argtypes == list(_abi.PROTOTYPES[n][1])
    assert callable(_lib.Handle.ft4_set_coherent) and callable(_lib.Handle.ft4_coherent) and callable(_lib.Handle.ft4_coh_info)
    assert synth.pack77("CQ", "K1ABC", "FN42") == cases.DEMOD_WORD
