"""Stored reference traces for tests/test_reference_crosscheck.py::test_default_subset: the frames of that test decoded by the REAL
reference (oracle/ref_harness.py), reduced to what crosscheck_frame compares -- the candidate list with scores and outcomes, the
fine-sync tweaks, LLRs and signal grids of every candidate that reached the fine sync, the first-pass no-AP LDPC inputs, every
osd_012 call (inputs and result), the unpack() call sequence and the message dicts -- one .npz per frame in tests/golden/crosscheck/.
The test then checks the oracle against these traces on any machine, with or without the reference tree.

    python oracle/gen_golden_crosscheck.py          (needs the reference tree, PYFT8_REFERENCE; ~5 s per frame)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from ref_harness import run_frame  # noqa: E402
from pyft8_amd import synth  # noqa: E402
import test_reference_crosscheck as X  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "crosscheck")
MESSAGE_KEYS = ("msg_tuple", "their_snr", "tsec", "fHz", "decode_notes")


def _f32(rows, width):
    return np.asarray(rows, np.float32).reshape(len(rows), *width)


def trace_arrays(tr):
    """The trace reduced to what crosscheck_frame reads, losslessly: fine-sync LLRs and grids only where it reads them
    (X.fine_arrays_read), osd_012 inputs that differ from the candidate's fine LLRs in a few positions (the a-priori bits of an AP
    pattern) as those positions and values (the layout stored_trace decodes)."""
    fine_idx = sorted(tr.fine)
    kept = [i for i in fine_idx if X.fine_arrays_read(bool(tr.fine[i]["stopped"]), tr.final[i]["h0_idx"])]
    row_of = {i: r for r, i in enumerate(kept)}
    bp = [c for c in tr.bp_calls if c["ipass"] == 0 and c["ap"] == "NoAP"]
    osd_base, osd_ndiff, osd_pos, osd_val, osd_full = [], [], [], [], []
    for c in tr.osd_calls:
        llr = np.asarray(c["llr_in"], np.float32)
        r = row_of.get(c["cand"])
        diff = np.nonzero(np.asarray(tr.fine[c["cand"]]["llr"], np.float32) != llr)[0] if r is not None else None
        if diff is not None and len(diff) < 64:
            osd_base.append(r), osd_ndiff.append(len(diff)), osd_pos.extend(diff), osd_val.extend(llr[diff])
        else:
            osd_base.append(-1), osd_ndiff.append(0), osd_full.append(llr)
    meta = {"final": [dict(f0_idx=f["f0_idx"], h0_idx=f["h0_idx"], score=f["score"], ipass=f["ipass"],
                           result=list(f["result"]) if f["result"] else None) for f in tr.final],
            "fine": [dict(idx=i, tweaks=tr.fine[i]["tweaks"], stopped=bool(tr.fine[i]["stopped"])) for i in fine_idx],
            "bp_cand": [c["cand"] for c in bp],
            "osd": [dict(cand=c["cand"], ipass=c["ipass"], ap=c["ap"], result=list(c["result"]) if c["result"] is not None else None)
                    for c in tr.osd_calls],
            "unpack": [[format(bits, "x"), res is not None, cand, ipass] for bits, res, cand, ipass in tr.unpack_calls],
            "messages": [{k: (list(m[k]) if k == "msg_tuple" else m[k]) for k in MESSAGE_KEYS} for m in tr.messages]}
    return {"meta": np.array(json.dumps(meta)),
            "fine_llr": _f32([tr.fine[i]["llr"] for i in kept], (174,)),
            "fine_sgrid": _f32([tr.fine[i]["signal_grid"] for i in kept], (79, 8)),
            "bp_llr": _f32([c["llr_in"] for c in bp], (174,)),
            "osd_base": np.array(osd_base, np.int16), "osd_ndiff": np.array(osd_ndiff, np.int16),
            "osd_pos": np.array(osd_pos, np.uint8), "osd_val": np.array(osd_val, np.float32),
            "osd_llr": _f32(osd_full, (174,))}


def check_stored(which, k, tr):
    """The stored file decodes to the live trace, bit for bit, wherever crosscheck_frame reads it."""
    st = X.stored_trace(which, k)
    same = lambda a, b: np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
    assert len(st.final) == len(tr.final) and len(st.fine) == len(tr.fine)
    for i, f in st.fine.items():
        if f["llr"] is not None:
            assert same(f["llr"], tr.fine[i]["llr"]) and same(f["signal_grid"], tr.fine[i]["signal_grid"]), i
    assert len(st.osd_calls) == len(tr.osd_calls)
    assert all(same(a["llr_in"], b["llr_in"]) for a, b in zip(st.osd_calls, tr.osd_calls))
    bp = [c for c in tr.bp_calls if c["ipass"] == 0 and c["ap"] == "NoAP"]
    assert all(same(a["llr_in"], b["llr_in"]) and a["cand"] == b["cand"] for a, b in zip(st.bp_calls, bp)) and len(st.bp_calls) == len(bp)


def main():
    os.makedirs(OUT, exist_ok=True)
    for which, k in X.DEFAULT_SUBSET:
        k, recipe, kw, base = X.frame_of_set(which, k)
        _, tr, _ = run_frame(synth.make_frame(base + k, **recipe), **kw)
        path = os.path.join(OUT, f"{which}_{k}.npz")
        np.savez_compressed(path, **trace_arrays(tr))
        check_stored(which, k, tr)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
