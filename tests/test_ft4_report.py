"""The float64 twin of the FT4 measured reports (pyft8_amd/ft4.py report) on its own: the accuracy recipe against
truth, the closed forms of the all-zero frame, the validity rule, the fixture of the GPU test (no crafted case is a near tie) and the
message dicts.  No GPU."""
import numpy as np
import pytest

import ft4_report_cases as cases
from pyft8_amd import ft4


# ----------------------------------------------------------------------------- 1. accuracy on the recipe
@pytest.fixture(scope="module")
def recipe_rows():
    """frames 0 .. 15 of the recipe through decode_twin and the twin's report -> rows (truth snr, errors of the report), and the same
    errors of the default fields"""
    rows, default = [], []
    for i in cases.TWIN_FRAMES:
        made = cases.recipe_frame(i)
        if made is None:
            continue
        x, truth = made
        by_word = {t["word"]: t for t in truth}
        seen = set()
        for r in ft4.decode_twin(x):
            t = by_word.get(r["word"])
            if t is None or r["word"] in seen:
                continue
            seen.add(r["word"])
            p = ft4.report(x, ft4.sig_from_record(r["f0"], r["h0"], r["tt"], r["ft"], r["word"]))
            assert p["flags"] & ft4.RP_MEASURED and not p["flags"] & ft4.RP_INVALID
            rows.append((t["snr"], p["snr_db"] - t["snr"], p["f_hz"] - t["f0"], 1e3 * (p["t_sec"] - t["t0"])))
            default.append((t["snr"], r["snr"] - t["snr"], ft4.BIN_HZ * r["f0"] + ft4.DF_HZ * r["ft"] - t["f0"],
                            1e3 * ((ft4.HOP * r["h0"] + ft4.DT_STEP * r["tt"]) / ft4.FS - t["t0"])))
    return rows, default


def test_twin_against_truth_on_the_recipe(recipe_rows):
    rows, default = recipe_rows
    s, d = cases.error_stats(rows), cases.error_stats(default)
    print("ft4 report twin   :", {k: round(v, 4) for k, v in s.items()})
    print("ft4 default fields:", {k: round(v, 4) for k, v in d.items()})
    assert s["n"] >= 80 and s["n_low"] >= 20 and s["n_high"] >= 20
    cases.check_bounds(s)
    # what the report is for: the default fields sit on the fine grid and read the SNR low
    assert s["f_rms"] < 0.25 * d["f_rms"] and s["t_std"] < 0.5 * d["t_std"] and abs(s["snr_high_mean"]) < abs(d["snr_high_mean"])


# ----------------------------------------------------------------------------- 2. closed forms
def test_all_zero_frame():
    i = [c[0] for c in cases.CASES].index("all zero")
    sig, r = cases.CASES[i][2], cases.twin(i)
    assert r["flags"] == ft4.RP_MEASURED | ft4.RP_EDGE_T | ft4.RP_EDGE_F
    assert not r["scores"].any() and r["score"] == 0.0 and r["on"] == 0.0 and r["off"] == 0.0
    assert r["snr_db"] == pytest.approx(10.0 * np.log10(1e-3 * (12000.0 / 576.0) / 2500.0), abs=1e-12) and round(r["snr_db"], 2) == -50.79
    assert r["t_sec"] == (sig["start"] - 36) / 12000.0
    assert r["f_hz"] == pytest.approx(sig["fq"] * 12000.0 / 4608.0 - 6 * 12000.0 / 18432.0, abs=1e-9)
    assert abs(r["f_hz"] - (sig["fq"] * 2.6042 - 3.9063)) < 0.02


def test_a_clean_signal_reads_its_own_numbers():
    """without noise the model is the signal: the peak is the centre of both axes, the parabolas stay inside a hundredth of a step, and
    the floor is far below (off comes from the signal's own leakage into the cells three tones away)"""
    w = cases.WORDS[0]
    x = ft4.frame_with_signals(1, [(w, 400 * ft4.DF_HZ, 0.5, 20.0)], noise=False)
    r = ft4.report(x, dict(start=6000, fq=400, tones=ft4.tones105(w)))
    assert r["flags"] == ft4.RP_MEASURED and r["tau"] == 0
    assert abs(r["f_hz"] - 400 * ft4.DF_HZ) < 0.01 * ft4.RP_DELTA_HZ and abs(r["t_sec"] - 0.5) < 0.06 / 12000.0
    assert r["snr_db"] > 35.0
    k = int(np.argmax(r["scores"]))
    assert divmod(k, 13) == (6, 6) and r["score"] == r["scores"][6, 6]


# ----------------------------------------------------------------------------- 3. validity
def test_invalid_below_32_symbols():
    w = cases.WORDS[1]
    x = cases.frame("strong")
    sig = dict(start=0, fq=576, tones=ft4.tones105(w))
    # symbols 1 .. q are whole inside n_have = 576 (q + 1) at tau = 0; the peak's tau moves the count by one at most
    for n_sym, want_ok in ((31, False), (34, True)):
        r = ft4.report(x, sig, n_have=576 * (n_sym + 1) + 36)
        assert r["n_valid"] in (n_sym - 1, n_sym), r["n_valid"]
        assert bool(r["flags"] & ft4.RP_INVALID) == (not want_ok)
        if not want_ok:
            assert r["flags"] == ft4.RP_MEASURED | ft4.RP_INVALID
            assert all(np.isnan(r[k]) for k in ("snr_db", "f_hz", "t_sec", "score"))
    r = ft4.report(x, dict(sig, start=6000), n_have=6000 + 36 + 576 * 33)      # exactly 32 whole symbols at tau <= 0 ... 36
    assert r["n_valid"] >= 32 or r["flags"] & ft4.RP_INVALID


def test_the_cases_show_what_they_are_for():
    for i, (name, _, sig, n_have) in enumerate(cases.CASES):
        r = cases.twin(i)
        if name == "noise only":                                            # a peak anywhere on the map, borders included
            assert r["flags"] & ft4.RP_MEASURED and not r["flags"] & ft4.RP_INVALID and r["snr_db"] < -18.0
            continue
        assert r["flags"] == cases.WANT_FLAGS.get(name, ft4.RP_MEASURED), (name, r["flags"])
        if cases.WANT_VALID.get(name) is not None:
            assert r["n_valid"] == cases.WANT_VALID[name], (name, r["n_valid"])
    by = {c[0]: cases.twin(i) for i, c in enumerate(cases.CASES)}
    assert by["f0 15 Hz"]["cells"].size == 309 and by["f0 5900 Hz"]["cells"].size == 309 and by["interior +10 dB"]["cells"].size == 618
    assert by["n_have 72000"]["n_valid"] < by["interior +10 dB"]["n_valid"] == 103
    assert abs(by["interior -14 dB"]["snr_db"] + 14.0) < 2.0 and abs(by["interior +10 dB"]["snr_db"] - 10.0) < 1.0
    assert abs(by["n_have 72000"]["snr_db"] - 10.0) < 1.0
    for name in ("start -0.3 s", "start 5.0 s", "f0 15 Hz", "f0 5900 Hz"):
        assert abs(by[name]["snr_db"]) < 1.0, (name, by[name]["snr_db"])


# ----------------------------------------------------------------------------- 4. the fixture: no near tie
def test_no_case_is_a_near_tie():
    for i, (name, *_rest) in enumerate(cases.CASES):
        r = cases.twin(i)
        P = np.sort(r["scores"].reshape(-1))
        if P[-1] == 0.0:
            assert name == "all zero"                                       # exact zeros: decided by the order of the trials alone
            continue
        lead = (P[-1] - P[-2]) / P[-1]
        print(f"ft4 report case {i} {name}: lead {lead:.3e}")
        assert lead >= cases.TIE_MARGIN, (name, lead)
        if r["flags"] & ft4.RP_INVALID:
            continue
        c = r["cells"]
        k = (len(c) - 1) // 4
        assert c[k - 1] < c[k] < c[k + 1], name


# ----------------------------------------------------------------------------- 5. message dicts
def _rows():
    from pyft8_amd import _lib
    m = np.zeros(2, _lib.MESSAGE_DTYPE)
    m["f"][0] = (b"CQ", b"K1ABC", b"FN42")
    m["f"][1] = (b"K1ABC", b"W9XYZ", b"-07")
    m["f0_idx"], m["h0_idx"], m["ttweak"], m["ftweak"], m["snr"] = (100, 150), (40, 50), (1, -2), (0, 2), (-3, 5)
    return m


def test_message_dicts_without_reports_are_todays():
    m = _rows()
    plain = ft4.message_dicts(m, 2, cyclestart_string="700101_000007.5")
    assert all("report" not in d for d in plain)
    assert set(plain[0]) == {"band", "tsec", "fHz", "msg_tuple", "their_snr", "their_tx_cycle", "all_txt_format", "cyclestart_string",
                             "decode_completed", "tweaks", "decode_notes", "mode"}
    from pyft8_amd import _lib
    rp = np.zeros(2, _lib.REPORT_DTYPE)
    rp[0] = (-3.25, 1041.5, 0.4825, 7.0, ft4.RP_MEASURED | ft4.RP_EDGE_T, 0)
    rp[1]["flags"] = ft4.RP_MEASURED | ft4.RP_INVALID
    rp[1]["snr_db"] = np.nan
    seen = []
    with_rp = ft4.message_dicts(m, 2, cyclestart_string="700101_000007.5", reports=rp, on_message=seen.append)
    assert with_rp[0]["report"] == {"snr": -3.25, "fHz": 1041.5, "tsec": pytest.approx(0.4825)} and with_rp[1]["report"] is None
    assert all(type(v) is float for v in with_rp[0]["report"].values())
    assert seen == with_rp                                                  # on_message sees the finished dict
    for a, b in zip(plain, with_rp):
        assert {k: v for k, v in b.items() if k not in ("report", "decode_completed")} == {k: v for k, v in a.items() if k != "decode_completed"}


# ----------------------------------------------------------------------------- 6. the receiver's side, on a handle that records
class RecordingHandle:
    def __init__(self):
        self.calls = []

    def ft4_staging_ptr(self):
        return 0x1000

    def ft4_report(self, ptr, sigs, n_have=90000, stages=False):
        from pyft8_amd import _lib
        self.calls.append((ptr, sigs[0].copy(), sigs[1].copy(), n_have))
        out = np.zeros(sigs[0].shape, _lib.REPORT_DTYPE)
        out["flags"] = ft4.RP_MEASURED
        out["snr_db"] = np.arange(out.size).reshape(out.shape)
        return out


class NoDevice:
    """a handle that may be created and closed and nothing else"""
    def __init__(self, cfg=None, device=0, max_frames=1):
        self.cfg, self.max_frames = cfg, int(max_frames)

    def set_ladder_mode(self, mode):
        pass

    def close(self):
        pass


def test_receiver_builds_one_signal_per_message(monkeypatch):
    from pyft8_amd import _lib
    from pyft8_amd.receiver import Receiver
    monkeypatch.setattr(_lib, "Handle", NoDevice)
    with pytest.raises(_lib.Ft8rxError, match="ft4_reports must be True or False"):
        Receiver("", None, ft4_reports="yes")
    w0, w1, w2 = cases.WORDS[:3]
    rec = np.zeros((2, 4), _lib.RECORD_DTYPE)
    for f, c, w, f0, h0, tt, ft in ((0, 1, w0, 96, 50, -2, 1), (0, 3, w1, 300, -3, 4, -2), (1, 0, w2, 144, 10, 0, 0)):
        rec[f, c]["msg_lo"], rec[f, c]["msg_hi"] = w & (2 ** 64 - 1), w >> 64
        rec[f, c]["f0_idx"], rec[f, c]["h0_idx"], rec[f, c]["ttweak"], rec[f, c]["ftweak"] = f0, h0, tt, ft
    msgs = np.zeros((2, 3), _lib.MESSAGE_DTYPE)
    msgs["cand"][0, :2] = (3, 1)                                            # the messages name their records, in their own order
    msgs["cand"][1, 0] = 0
    mcnt = np.array([2, 1], np.int32)
    h = RecordingHandle()
    off = Receiver("", None)
    assert off.ft4_reports is False and off._ft4_measure(h, 2, rec, msgs, mcnt) is None and h.calls == [] and off._ft4_rp(None, 0) == {}
    on = Receiver("", None, ft4_reports=True)
    rp = on._ft4_measure(h, 2, rec, msgs, mcnt, n_have=72000)
    (ptr, sigs, counts, n_have), = h.calls
    assert ptr == 0x1000 and n_have == 72000 and counts.tolist() == [2, 1] and sigs.shape == (2, 2)
    assert [len(r) for r in rp] == [2, 1] and rp[0]["snr_db"].tolist() == [0.0, 1.0] and rp[1]["snr_db"].tolist() == [2.0]
    want = [ft4.sig_from_record(300, -3, 4, -2, w1), ft4.sig_from_record(96, 50, -2, 1, w0), ft4.sig_from_record(144, 10, 0, 0, w2)]
    for got, sg in zip((sigs[0, 0], sigs[0, 1], sigs[1, 0]), want):
        assert int(got["start"]) == sg["start"] and int(got["fq"]) == sg["fq"] and got["tones"].tolist() == sg["tones"]
    assert on._ft4_rp(rp, 1)["reports"] is rp[1]
    del h.calls[:]
    assert [len(r) for r in on._ft4_measure(h, 2, rec, msgs, np.zeros(2, np.int32))] == [0, 0] and h.calls == []      # nothing to measure: no call
