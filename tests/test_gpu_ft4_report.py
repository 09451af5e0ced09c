"""FT4 measured reports on the GPU (csrc/kernels/ft4_report.hpp) against the float64 twin pyft8_amd/ft4.py on the
fixtures of tests/ft4_report_cases.py: the crafted cases stage by stage, the byte-for-byte properties, the whole path through
Receiver(ft4_reports=True), and what the feature leaves alone.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import ft4_report_cases as cases
from pyft8_amd import _lib, ft4, synth
from pyft8_amd.receiver import Receiver, decode_frames_ft4

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle(max_frames=3)
    yield h
    h.close()


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b)) if float(b) != 0.0 else abs(float(a))


# ----------------------------------------------------------------------------- 1. the cases against the twin
def test_cases_against_the_twin(handle):
    worst = dict(scores=0.0, on=0.0, off=0.0, f_hz=0.0, t_sec=0.0, snr_db=0.0)
    done = set()
    for n_have, audio, sigs, counts, where in cases.calls():
        assert audio.shape == (3, 90000) and sigs.shape == (3, 5) and counts[1] == 0
        rep, sc, oo = handle.ft4_report(audio, (sigs, counts), n_have=n_have, stages=True)
        for f in range(3):                                                  # beyond the count: all zero
            assert not rep[f, counts[f]:].tobytes().strip(b"\0") and not sc[f, counts[f]:].any() and not oo[f, counts[f]:].any()
        for (f, k), i in where.items():
            name, want, got = cases.CASES[i][0], cases.twin(i), rep[f, k]
            done.add(i)
            assert int(got["flags"]) == want["flags"], (name, int(got["flags"]), want["flags"])
            assert int(got["pad"]) == 0
            top = float(want["scores"].max())
            e = dict(scores=float(np.abs(sc[f, k] - want["scores"]).max()) / top if top > 0 else float(np.abs(sc[f, k]).max()))
            if want["flags"] & ft4.RP_INVALID:
                assert all(np.isnan(got[key]) for key in ("snr_db", "f_hz", "t_sec", "score")) and np.isnan(oo[f, k]).all(), name
            else:
                e.update(on=_rel(oo[f, k, 0], want["on"]), off=_rel(oo[f, k, 1], want["off"]), f_hz=abs(float(got["f_hz"]) - want["f_hz"]),
                         t_sec=abs(float(got["t_sec"]) - want["t_sec"]), snr_db=abs(float(got["snr_db"]) - want["snr_db"]))
                assert _rel(got["score"], want["score"]) <= cases.SCORE_BOUND and float(got["score"]) == float(sc[f, k].max())
            print(f"ft4 report case {i} {name}: flags {int(got['flags'])}, " + ", ".join(f"{key} {v:.3e}" for key, v in e.items()))
            for key, v in e.items():
                worst[key] = max(worst[key], v)
    assert done == set(range(len(cases.CASES)))
    print("ft4 report worst: " + ", ".join(f"{key} {v:.3e}" for key, v in worst.items()))
    assert worst["scores"] <= cases.SCORE_BOUND and worst["on"] <= cases.ON_BOUND and worst["off"] <= cases.OFF_BOUND
    assert worst["f_hz"] <= cases.F_BOUND and worst["t_sec"] <= cases.T_BOUND and worst["snr_db"] <= cases.SNR_BOUND


# ----------------------------------------------------------------------------- 2. byte for byte
def test_same_bytes_again_alone_and_beside_an_idle_row(handle):
    audio, sigs, counts = cases.batch()
    assert counts.tolist() == [5, 0, 3]
    first = handle.ft4_report(audio, (sigs, counts), stages=True)
    assert (first[0]["flags"][0] & ft4.RP_MEASURED).all() and (first[0]["flags"][2, :3] & ft4.RP_MEASURED).all()
    again = handle.ft4_report(audio, (sigs, counts), stages=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    # a row with count 0: nothing, whatever its slots hold
    assert not first[0][1].tobytes().strip(b"\0") and not first[1][1].any() and not first[2][1].any()
    junk = sigs.copy()
    junk[1] = sigs[0]
    junk[2, 3:] = sigs[0, :2]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, handle.ft4_report(audio, (junk, counts), stages=True)))
    # a frame alone, and one of its signals alone: the bytes they have in the batch
    for f in (0, 2):
        alone = handle.ft4_report(audio[f:f + 1], (sigs[f:f + 1], counts[f:f + 1]), stages=True)
        assert all(a.tobytes() == b[f:f + 1].tobytes() for a, b in zip(alone, first))
    one = handle.ft4_report(audio[2:3], (sigs[2:3, 1:2], np.array([1], np.int32)), stages=True)
    assert all(a.tobytes() == b[2:3, 1:2].tobytes() for a, b in zip(one, first))
    # through the device pointer of an FT4 batch's staging buffer: the same bytes
    handle.ft4_decode(audio)
    assert handle.ft4_report(handle.ft4_staging_ptr(), (sigs, counts)).tobytes() == first[0].tobytes()


# ----------------------------------------------------------------------------- 3. the whole path
@pytest.fixture(scope="module")
def whole():
    made = [ft4.make_frame(300 + i, n_signals=5, snr_range=(-10.0, 8.0), min_sep_hz=300.0, return_truth=True) for i in range(3)]
    audio = np.stack([m[0] for m in made])
    plain = Receiver("", None, max_frames=3)
    base = plain.decode_frames_ft4(audio)
    plain.close()
    return audio, [m[1] for m in made], base


def _strip(d):
    return {k: v for k, v in d.items() if k not in ("report", "decode_completed")}


def _errors(out, truth):
    rows = []
    for f, dicts in enumerate(out):
        by_text = {t["msg"]: t for t in truth[f]}
        for d in dicts:
            assert "report" in d
            t = by_text.get(" ".join(x for x in d["msg_tuple"] if x))
            if t is None:
                continue
            assert d["report"] is not None and set(d["report"]) == {"snr", "fHz", "tsec"} and all(type(v) is float for v in d["report"].values())
            rows.append((t["snr"], d["report"]["snr"] - t["snr"], d["report"]["fHz"] - t["f0"], 1e3 * (d["report"]["tsec"] - t["t0"])))
    return rows


@pytest.mark.parametrize("kw", [{}, {"ft4_passes": 2}, {"ft4_coherent": True}], ids=["plain", "passes2", "coherent"])
def test_whole_path(whole, kw):
    audio, truth, base = whole
    rx = Receiver("", None, max_frames=3, ft4_reports=True, **kw)
    seen = []
    rx.on_message = seen.append
    out = rx.decode_frames_ft4(audio)
    assert rx._handle(3).ft4_report_info()["workspace_bytes"] > 0
    rx.close()
    assert all("report" in d for d in seen) and len(seen) == sum(len(o) for o in out)
    if kw:
        off = Receiver("", None, max_frames=3, **kw)
        base = off.decode_frames_ft4(audio)
        assert off._handle(3).ft4_report_info()["workspace_bytes"] == 0
        off.close()
    assert [[_strip(d) for d in o] for o in out] == [[_strip(d) for d in o] for o in base]
    assert all("report" not in d for o in base for d in o)
    rows = _errors(out, truth)
    s = cases.error_stats(rows)
    print(f"ft4 report whole path {kw}: {s}")
    assert s["n"] >= 12
    cases.check_bounds(s)
    if kw.get("ft4_passes"):
        sub = [d for o in out for d in o if "_SUB" in d["decode_notes"]]
        print(f"ft4 report: {len(sub)} _SUB messages")
        assert all("report" in d for d in sub)


def test_later_pass_messages_carry_a_report():
    """a crowded frame (16 signals in 900 Hz: the twin's second pass brings six more): every "_SUB" message is measured -- on the
    residual its pass decoded, so its frequency and time lie inside the scan's window around its own record's"""
    audio = ft4.make_frame(1001, n_signals=16, snr_range=(-12, 10), freq_range=(300, 1200), t0_range=(0.2, 1.2), min_sep_hz=25)[None]
    out = decode_frames_ft4(audio, ft4_reports=True, ft4_passes=2)[0]
    base = decode_frames_ft4(audio, ft4_passes=2)[0]
    assert [_strip(d) for d in out] == [_strip(d) for d in base]
    sub = [d for d in out if "_SUB" in d["decode_notes"]]
    print(f"ft4 report: {len(out)} messages, {len(sub)} of a later pass")
    assert len(sub) >= 1 and len(out) - len(sub) >= 1
    for d in out:
        assert d["report"] is not None
        assert abs(d["report"]["fHz"] - d["fHz"]) <= 6.5 * ft4.RP_DELTA_HZ and abs(d["report"]["tsec"] - d["tsec"]) <= 42.5 / 12000.0


def test_module_level_entry_takes_the_setting(whole):
    audio, _, base = whole
    out = decode_frames_ft4(audio[:1], ft4_reports=True)
    assert [_strip(d) for d in out[0]] == [_strip(d) for d in base[0]] and all(d["report"] is not None for d in out[0]) and out[0]


# ----------------------------------------------------------------------------- 4. what stays the same
def test_setting_off_calls_nothing_new(whole):
    audio, _, base = whole
    with pytest.raises(_lib.Ft8rxError, match="ft4_reports must be True or False"):
        Receiver("", None, ft4_reports=1)
    calls = []

    class Spy:
        def __init__(self, h):
            self._h = h

        def __getattr__(self, name):
            calls.append(name)
            return getattr(self._h, name)

    for on in (False, True):
        rx = Receiver("", None, max_frames=3, **({"ft4_reports": True} if on else {}))
        h = rx._handle(3)
        del calls[:]
        rx._handle = lambda B, h=h: Spy(h)
        out = rx.decode_frames_ft4(audio)
        info = h.ft4_report_info()["workspace_bytes"]
        rx.close()
        if on:
            assert calls == ["ft4_set", "ft4_set_range", "ft4_decode", "ft4_report", "ft4_staging_ptr"] or calls == ["ft4_set", "ft4_set_range", "ft4_decode", "ft4_staging_ptr", "ft4_report"]
            assert info > 0
        else:
            assert calls == ["ft4_set", "ft4_set_range", "ft4_decode"] and info == 0
            assert [[_strip(d) for d in o] for o in out] == [[_strip(d) for d in o] for o in base]


def test_info_and_the_other_workspaces():
    h = _lib.Handle(max_frames=2)
    audio, sigs, counts = cases.batch()
    assert h.ft4_report_info()["workspace_bytes"] == 0
    h.ft4_decode(audio[:2])
    before = (h.ft4_info()["workspace_bytes"], h.ft4_sub_info()["workspace_bytes"])
    assert h.ft4_report_info()["workspace_bytes"] == 0
    h.ft4_report(h.ft4_staging_ptr(), (sigs[:2], counts[:2]))
    got = h.ft4_report_info()["workspace_bytes"]
    assert 1_800_000 < got < 2_000_000                                       # 0.95 MB per frame of max_frames
    assert (h.ft4_info()["workspace_bytes"], h.ft4_sub_info()["workspace_bytes"]) == before
    h.ft4_report(h.ft4_staging_ptr(), (sigs[:2], counts[:2]))
    assert h.ft4_report_info()["workspace_bytes"] == got
    h.close()


def test_ft8_after_an_ft4_report_is_a_fresh_handles():
    a8 = synth.make_frame(11, n_signals=6, snr_range=(-10.0, 5.0))[None]
    fresh = _lib.Handle(max_frames=1)
    want = fresh.decode_batch(a8)
    fresh.close()
    h = _lib.Handle(max_frames=1)
    audio, sigs, counts = cases.batch()
    h.ft4_report(audio[:1], (sigs[:1], counts[:1]))
    got = h.decode_batch(a8)
    h.close()
    n, ne = int(want[1][0]), int(want[3][0])                                # records up to the count; the event log's order is the run's
    assert n > 0 and ne > 0 and int(got[1][0]) == n and int(got[3][0]) == ne and got[0][0, :n].tobytes() == want[0][0, :n].tobytes()
    key = lambda ev: sorted(e.tobytes() for e in ev)
    assert key(got[2][0, :ne]) == key(want[2][0, :ne])


def test_reports_true_is_still_refused_for_ft4(whole):
    rx = Receiver("", None, max_frames=1, reports=True)
    with pytest.raises(_lib.Ft8rxError, match="reports"):
        rx.decode_frames_ft4(whole[0][:1])
    rx.close()
    rx = Receiver("", None, max_frames=1, reports=True, ft4_reports=True)
    with pytest.raises(_lib.Ft8rxError, match="reports"):
        rx.decode_frames_ft4(whole[0][:1])
    rx.close()


def test_refusals_by_name(handle):
    audio, sigs, counts = cases.batch()

    def bad(match, s=sigs, c=counts, **kw):
        with pytest.raises(_lib.Ft8rxError, match=match):
            handle.ft4_report(audio, (s, c), **kw)

    s = sigs.copy(); s[2, 1]["tones"][50] = 4
    bad(r"signal 1 of frame 2: tone 4 of symbol 50 is above 3", s)
    s = sigs.copy(); s[0, 4]["fq"] = 4608
    bad(r"signal 4 of frame 0: fq 4608 outside \[0, 4608\)", s)
    s = sigs.copy(); s[0, 0]["fq"] = -1
    bad(r"fq -1 outside \[0, 4608\)", s)
    s = sigs.copy(); s[0, 2]["start"] = (1 << 20) + 1
    bad(r"signal 2 of frame 0: \|start\| 1048577 above 2\^20", s)
    s = sigs.copy(); s[2, 0]["start"] = -(1 << 20) - 1
    bad(r"\|start\| -1048577 above 2\^20", s)
    bad(r"n_have 575 outside \[576, 90000\]", n_have=575)
    bad(r"n_have 90001 outside \[576, 90000\]", n_have=90001)
    bad(r"counts\[0\] = 6 outside \[0, 5\]", c=np.array([6, 0, 3], np.int32))
    with pytest.raises(_lib.Ft8rxError, match="max_sigs 0 is below 1"):
        handle.ft4_report(audio, (np.zeros((3, 0), _lib.FT4_SUBSIG_DTYPE), np.zeros(3, np.int32)))
    # a bad signal beyond its frame's count is not looked at; and nothing above left a trace: the next call is the first one's bytes
    s = sigs.copy(); s[2, 4]["fq"] = 9999; s[1, 0]["tones"][:] = 7
    assert handle.ft4_report(audio, (s, counts)).tobytes() == handle.ft4_report(audio, (sigs, counts)).tobytes()
