"""The opt-in steps on one long-lived handle: the library refuses exactly the pairs that pyft8_amd/optins.py
tables, naming both, and the workspaces each step creates on first use -- in whatever order the steps come -- give the results of a
fresh handle that has only that step."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

from conftest import load_golden
from pyft8_amd import _lib, optins, synth
from pyft8_amd import recall as R

pytestmark = pytest.mark.gpu

# the library's entry point of each setting, and the name its refusals use for it (csrc/optins.hpp)
ENTRY = {optins.PACKED: "ft8rx_set_packed_output", optins.MSG_TYPES: "ft8rx_set_msg_types", optins.AP_CALLS: "ft8rx_set_ap_calls",
         optins.RECALL: "ft8rx_set_recall", optins.WEAK: "ft8rx_set_weak", optins.REPORTS: "ft8rx_set_reports"}
C_NAME = dict(ENTRY, **{optins.PACKED: "the packed output (ft8rx_set_packed_output)", optins.MSG_TYPES: "msg_types != 0"})


def _set_packed(h, bufs, cap):
    """The library's own call: _lib.Handle.set_packed_output answers msg_types != 0 itself, before the library is asked."""
    L = h._L
    p = [ctypes.c_void_p(b.ctypes.data) if b is not None else None for b in bufs]
    h._chk(L.ft8rx_set_packed_output(h._h, p[0], p[1], ctypes.c_uint64(cap)), "ft8rx_set_packed_output")


def test_optin_pairs_are_refused_as_tabled():
    h = _lib.Handle(max_frames=1)
    try:
        cap = _lib.packed_capacity(1)
        bufs = (h.pinned_bytes(cap), h.pinned_bytes(cap))
        entry = R._entry(synth.pack77("K1ABC", "W9XYZ", "-10"), 300, 10)
        on = {optins.PACKED: lambda: _set_packed(h, bufs, cap), optins.MSG_TYPES: lambda: h.set_msg_types(_lib.MT_ALL),
              optins.AP_CALLS: lambda: h.set_ap_calls("K1ABC", None), optins.RECALL: lambda: h.set_recall([[entry]]),
              optins.WEAK: lambda: h.set_weak(True), optins.REPORTS: lambda: h.set_reports(True)}
        off = {optins.PACKED: lambda: _set_packed(h, (None, None), 0), optins.MSG_TYPES: lambda: h.set_msg_types(0),
               optins.AP_CALLS: lambda: h.set_ap_calls(None, None), optins.RECALL: lambda: h.set_recall(None),
               optins.WEAK: lambda: h.set_weak(False), optins.REPORTS: lambda: h.set_reports(False)}
        assert set(on) == set(off) == set(optins.SETTINGS)
        refused = 0
        for first in optins.SETTINGS:
            for second in optins.SETTINGS:
                on[first]()
                if optins.conflict(second, {first}) is None:
                    on[second]()                                        # (second == first: set again)
                else:
                    with pytest.raises(_lib.Ft8rxError) as e:
                        on[second]()
                    assert f"{ENTRY[second]}: not supported together with {C_NAME[first]}" in str(e.value), (first, second, str(e.value))
                    refused += 1
                for s in optins.SETTINGS:                               # turning off is never refused, set or not
                    off[s]()
        assert refused == 20
    finally:
        h.close()


def _ev_sorted(ev, n):
    # (the order of a frame's event log is whatever the kernels' atomics give: common.hpp)
    return np.sort(ev[:n], order=["cand", "ipass", "slot", "seq"]).tobytes()


def _same_batch(a, b, what):
    (rec, cnt, ev, evc), (rec2, cnt2, ev2, evc2) = a, b
    assert np.array_equal(cnt, cnt2) and np.array_equal(evc, evc2) and cnt.sum() > 0, what
    for f in range(len(cnt)):
        assert rec[f, :cnt[f]].tobytes() == rec2[f, :cnt2[f]].tobytes(), (what, f)
        ne = min(int(evc[f]), _lib.EVENT_CAP)
        assert _ev_sorted(ev[f], ne) == _ev_sorted(ev2[f], ne), (what, f)


def _step(h, audio, step, sigs=None, prev=None):
    """One step on handle h, its setting turned off again afterwards -> (batch results, what the step adds, as bytes)."""
    B = len(audio)
    if step == "plain":
        return h.decode_batch(audio), b""
    if step == "reports":
        h.set_reports(True)
        res = h.decode_batch(audio)
        extra = h.fetch_reports(B).tobytes()
        h.set_reports(False)
        return res, extra
    if step == "recall":
        h.set_recall(prev)
        res = h.decode_batch(audio)                                    # (the batch consumes the setting)
        rrec, rcnt = h.fetch_recall(B)
        return res, rcnt.tobytes() + b"".join(rrec[f, :rcnt[f]].tobytes() for f in range(B))
    if step == "weak":
        h.set_weak(True)
        res = h.decode_batch(audio)
        h.set_weak(False)
        return res, b""
    if step == "msg_types":
        h.set_msg_types(_lib.MT_ALL)
        res = h.decode_batch(audio)
        h.set_msg_types(0)
        return res, b""
    if step == "packed":
        cap = _lib.packed_capacity(B)
        bufs = (h.pinned_bytes(cap), h.pinned_bytes(cap))
        h.set_packed_output(bufs[0].ctypes.data, bufs[1].ctypes.data, cap, keep=bufs)
        res = h.decode_batch(audio)
        which, hdr = h.packed_results()
        packed = bufs[which][:hdr["bytes"]].tobytes()
        h.set_packed_output(None, None, 0)
        # the packed bytes are this batch's own results in the packed layout (event order included); across handles the batches
        # are compared like every other step's
        assert not hdr["overflow"] and packed == _lib.pack_results(*res).tobytes()
        return res, np.int64(hdr["bytes"]).tobytes()
    refine = int(step[-1])                                             # "subtract0" .. "subtract3"
    res = h.decode_batch(audio)                                        # leaves the frames in the handle's staging buffer
    sigs = (sigs[0].copy(), sigs[1])                                   # (a refining sweep writes the new origins back into its list)
    resid, origins = h.subtract(h.staging_ptr(), B, sigs, return_float=True, refine=refine, return_origins=True)
    left = h.download_audio(h.staging_ptr(), B)
    assert np.abs(resid - audio).max() > 0
    return res, resid.tobytes() + left.tobytes() + np.array(origins, np.float64).tobytes()


STEPS = ["plain", "reports", "recall", "weak", "msg_types", "packed", "subtract0", "subtract1", "subtract2", "subtract3"]


def test_first_use_in_any_order_gives_a_fresh_handles_results():
    audio = np.stack([load_golden("test_08")[0], load_golden("test_09")[0]])
    B = len(audio)
    h = _lib.Handle(max_frames=B)
    try:
        plain = h.decode_batch(audio)
        rec, cnt, ev, evc = plain
        msgs, mcnt = _lib.package_batch(rec, cnt, ev, evc)
        assert (mcnt > 0).all()
        # one decoded signal per frame to subtract (the strongest), and a recall set at the positions of four decoded records
        arr, n = _lib.subtraction_list(msgs, mcnt, rec, -100)
        best = [int(np.argmax(msgs["snr"][f, :mcnt[f]])) for f in range(B)]
        sigs = (np.stack([arr[f, best[f]:best[f] + 1] for f in range(B)]), np.ones(B, np.int32))
        prev = []
        for f in range(B):
            dec = [r for r in rec[f, :cnt[f]] if r["status"] == _lib.ST_DECODED][:4]
            prev.append([R._entry(int(r["msg_lo"]) | (int(r["msg_hi"]) << 64), int(r["f0_idx"]), int(r["h0_idx"]), int(r["ttweak"]),
                                  int(r["ftweak"])) for r in dec])
            assert len(prev[f]) == 4
        for step in STEPS:
            got = _step(h, audio, step, sigs, prev)
            fresh_h = _lib.Handle(max_frames=B)
            try:
                want = _step(fresh_h, audio, step, sigs, prev)
            finally:
                fresh_h.close()
            _same_batch(got[0], want[0], step)
            assert got[1] == want[1], step
            if step not in ("weak", "msg_types", "recall"):             # those change the ladder's own results; the others must not
                _same_batch(got[0], plain, step)
    finally:
        h.close()
