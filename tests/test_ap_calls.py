"""A-priori calls (ipass 7, ft8rx_set_ap_calls) on the host: c28 packing and pattern layouts against synth, the refusals, the
Python plumbing, and the replay of ipass-7 records and events by both packagers.  No GPU needed."""
import random

import numpy as np
import pytest

from pyft8_amd import _lib, synth
from pyft8_amd import messages as M
from pyft8_amd.receiver import config_from_kwargs, set_ap_calls_cfg

MY, DX = "K1ABC", "W9XYZ"


def _c28_of(bits, k, first):
    return int("".join(str(int(b)) for b in bits[k][first:first + 28]), 2)


def test_c28_matches_synth():
    rng = np.random.default_rng(11)
    for _ in range(3000):
        a, b = synth.random_call(rng), synth.random_call(rng)
        bits, mask = _lib.ap_patterns(a, b)
        assert _c28_of(bits, 1, 0) == synth.pack_c28(a) and _c28_of(bits, 1, 29) == synth.pack_c28(b), (a, b)
        assert _c28_of(bits, 2, 0) == synth.pack_c28("CQ") and _c28_of(bits, 2, 29) == synth.pack_c28(b)


@pytest.mark.parametrize("bad", ["", "K1abc", "CQ", "DE", "QRZ", "K1ABC/P", "<K1ABC>", "A1BCDE", "K 1AB", " K1AB", "K1AB ",
                                 "TOOLONG1", "AB", "K1A2B", "1234", "ABCD", "K1ABC;"])
def test_refuses_non_standard(bad):
    if bad == "":
        _lib.ap_patterns(bad, None)          # "" = unset
        return
    with pytest.raises(_lib.Ft8rxError, match="my_call"):
        _lib.ap_patterns(bad, DX)
    with pytest.raises(_lib.Ft8rxError, match="dx_call"):
        _lib.ap_patterns(MY, bad)


def _word_bits(w):
    return np.array([(w >> (76 - i)) & 1 for i in range(77)], np.uint8)


def _cw_bits(w):
    cw = synth.encode174(w)
    return np.array([(cw >> (173 - i)) & 1 for i in range(174)], np.uint8)


def test_pattern_layouts():
    bits, mask = _lib.ap_patterns(MY, DX)
    partial = {0: (synth.pack77(MY, DX, "-15"), 29), 1: (synth.pack77(MY, DX, "-15"), 58), 2: (synth.pack77("CQ", DX, "FN42"), 58)}
    for k, (w, nk) in partial.items():
        known = np.array([i < nk or 74 <= i < 77 for i in range(174)])
        assert np.array_equal(mask[k].astype(bool), known)
        assert np.array_equal(bits[k][known], _word_bits(w)[known[:77]])
        assert not bits[k][~known].any()
        assert bits[k][28] == 0 and list(bits[k][74:77]) == [0, 0, 1]       # r1 = 0, i3 = 001
    for k, extra in ((3, "RRR"), (4, "73"), (5, "RR73")):
        assert mask[k].all() and np.array_equal(bits[k], _cw_bits(synth.pack77(MY, DX, extra)))
    b1, m1 = _lib.ap_patterns(MY, None)
    assert m1[0].any() and not m1[1:].any() and np.array_equal(b1[0], bits[0])
    b2, m2 = _lib.ap_patterns(None, DX)
    assert m2[2].any() and not m2[[0, 1, 3, 4, 5]].any() and np.array_equal(b2[2], bits[2])
    assert not _lib.ap_patterns(None, "")[1].any()


def test_config_plumbing():
    unset = config_from_kwargs()
    assert unset.ap_my_call is None and unset.ap_dx_call is None and unset.ap_max_hd is None
    c = config_from_kwargs(my_call=MY, dx_call=DX, ap_max_hd=30)
    assert (c.ap_my_call, c.ap_dx_call, c.ap_max_hd) == (MY, DX, 30)
    assert bytes(c) == bytes(unset)                      # ft8rx_config itself is unchanged: the calls are handle settings
    set_ap_calls_cfg(c, "", None)
    assert c.ap_my_call is None and c.ap_dx_call is None
    with pytest.raises(_lib.Ft8rxError, match="my_call"):
        config_from_kwargs(my_call="k1abc")
    with pytest.raises(_lib.Ft8rxError, match="msg_types"):
        config_from_kwargs(my_call=MY, msg_types="all")
    with pytest.raises(_lib.Ft8rxError, match="ap_max_hd"):
        config_from_kwargs(my_call=MY, ap_max_hd=0)


def _frame(rng):
    """Synthetic records / events of one frame: ipass 0..6 decodes, EXHAUSTED ones, and ipass-7 decodes of every method with
    earlier CRC-passing calls of other patterns in the log."""
    n = 12
    rec = np.zeros(n, _lib.RECORD_DTYPE)
    ev = []
    rec["f0_idx"] = np.arange(n) * 40 + 100
    rec["h0_idx"] = 10
    rec["grid_sd"] = rng.random(n) * 5 + 5
    rec["fine_sd"] = rng.random(n) * 5 + 5
    calls = ["N0CALL", "VE3ABC", "G4XYZ", "JA1XYZ", "AA9ZZ", "KB2QQ"]
    for i in range(n):
        w = synth.pack77(calls[i % 6], calls[(i + 1) % 6], f"{i - 20:+03d}")
        kind = i % 4
        r = rec[i]
        if kind == 0:                                                 # the reference's ladder (ipass 4, BP)
            r["status"], r["ipass"], r["ap"], r["method"], r["n_its"] = _lib.ST_DECODED, 4, 0, _lib.M_LDPC_B, 3
            ev.append((i, 4, 0, 4, w))
        elif kind == 1:
            r["status"] = _lib.ST_EXHAUSTED
        else:                                                         # ipass 7
            ap = int(rng.integers(5, 11))
            method = _lib.M_AP_CODEWORD if ap >= 8 else (_lib.M_LDPC_B if kind == 2 else _lib.M_OSD)
            n_its = 0 if method == _lib.M_AP_CODEWORD else int(rng.integers(0, 20))
            r["status"], r["ipass"], r["ap"], r["method"], r["n_its"] = _lib.ST_DECODED, 7, ap, method, n_its
            slot = 2 * ap + (1 if method == _lib.M_OSD else 0)
            seq = n_its + 1 if method == _lib.M_LDPC_B else n_its
            ev.append((i, 7, slot, seq, w))
            ev.append((i, 7, 10, 5, synth.pack77("KH6ABC", "W9XYZ", "73")))          # an earlier pattern's call: replayed first
            ev.append((i, 7, 21, 0, synth.pack77("ZZ9ZZZ", "W9XYZ", "RRR")))        # after the accepted one: never replayed
        r["msg_lo"], r["msg_hi"] = w & ((1 << 64) - 1), w >> 64
    events = np.zeros(_lib.EVENT_CAP, _lib.EVENT_DTYPE)
    rng.shuffle(ev)
    for j, (c, ip, sl, sq, w) in enumerate(ev):
        events[j] = (w & ((1 << 64) - 1), w >> 64, c, ip, sl, sq, 1)
    return rec, events, len(ev)


def test_ipass7_packaging_python_and_native():
    rng = np.random.default_rng(3)
    B, n = 8, 12
    rec = np.zeros((B, n), _lib.RECORD_DTYPE)
    ev = np.zeros((B, _lib.EVENT_CAP), _lib.EVENT_DTYPE)
    cnt, evc = np.full(B, n, np.int32), np.zeros(B, np.int32)
    for f in range(B):
        rec[f], ev[f], evc[f] = _frame(rng)
    msgs, mcnt = _lib.package_batch(rec, cnt, ev, evc)
    for f in range(B):
        py = M.package_frame(rec[f], n, ev[f], evc[f], ap=True)
        nat = M.message_dicts(msgs[f], mcnt[f], ap=True)
        assert [m["msg_tuple"] for m in py] == [m["msg_tuple"] for m in nat]
        assert [m["decode_notes"] for m in py] == [m["decode_notes"] for m in nat]
        assert [m["ap"] for m in py] == [m["ap"] for m in nat]
        n7 = sum(1 for r in rec[f] if r["ipass"] == 7)
        assert sum(1 for m in py if m["ap"] in M.AP_CALL_NAMES) == n7 > 0
        # the ipass-7 messages come last: round 7 of the replay
        assert all(m["ap"] in M.AP_CALL_NAMES for m in py[-n7:])
        # replay: the earlier pattern's call entered the hash table, the later one did not
        t = M.CallHashes()
        M.package_frame(rec[f], n, ev[f], evc[f], table=t)
        assert "KH6ABC" in t.by_call and "ZZ9ZZZ" not in t.by_call
        assert all("ap" not in m for m in M.package_frame(rec[f], n, ev[f], evc[f]))
