"""FT4 subtraction passes on the GPU (csrc/kernels/ft4_sub.hpp) against the float64 twin pyft8_amd/ft4.py on the
fixtures of tests/ft4_sub_cases.py: the model, bins and trial energies of crafted signals, the refine decisions, the residual of a
batch, the whole path through Receiver(ft4_passes=...), and what the feature leaves alone.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import ft4_cases
import ft4_sub_cases as cases
from pyft8_amd import _lib, ft4, synth
from pyft8_amd.receiver import Receiver, decode_frames_ft4

pytestmark = pytest.mark.gpu
# The probe against the twin over the twelve crafted signals; each bound is 4 x the worst value of the first run on an MI355X, rounded
# up to one digit (profiles/ft4_subtract_notes.md):
#   model   max |s - s64| over the 60480 samples (the model's amplitude is 1): measured 8.082e-7 (the place where nothing is planted,
#           3600 Hz; every case lies between 6.1e-7 and 8.1e-7: the hardware sine and cosine)
#   bins    max |A - A64| / max |A64| over the 41 bins: measured 2.436e-6 (the same case: its largest bin is noise; the planted signals
#           6.8e-8 .. 5.5e-7)
#   energy  max |E - E64| / max E64 over the 13 trials: measured 1.323e-6 (the same case; the planted signals 1.2e-7 .. 5.1e-7)
MODEL_BOUND = 4e-6
BINS_BOUND = 1e-5
ENERGY_BOUND = 6e-6
# The float32 residual of the batch against the twin at the GPU's own starts: max |r - r64| in counts; measured 5.171e-3 (frame 1;
# 2.781e-6 of the frame's RMS at worst, frame 2 -- the bound ft8rx_subtract is held to, 1e-4 of the RMS, holds on top)
RESIDUAL_BOUND = 3e-2


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle(max_frames=4)
    yield h
    h.close()


def _device(audio):
    return torch.from_numpy(np.ascontiguousarray(audio, np.int16).copy()).cuda()


# ----------------------------------------------------------------------------- 1. probe
def test_probe_against_the_twin(handle):
    audio, frame, sigs, _ = cases.probe_cases()
    models, bins, en, _ = cases.probe_twin()
    got = handle.ft4_sub_probe(audio, frame, cases.subsig_array(sigs), want_model=True)
    worst = [0.0, 0.0, 0.0]
    for i, p in enumerate(cases.PROBE):
        em = float(np.abs(got["model"][i].astype(np.complex128) - models[i]).max())
        top, etop = float(np.abs(bins[i]).max()), float(en[i].max())
        eb = float(np.abs(got["bins"][i] - bins[i]).max()) / top if top > 0 else 0.0
        ee = float(np.abs(got["energy"][i] - en[i]).max()) / etop if etop > 0 else 0.0
        print(f"ft4 sub probe {i} {p}: model {em:.3e}, bins {eb:.3e}, energy {ee:.3e}")
        worst = [max(a, b) for a, b in zip(worst, (em, eb, ee))]
        if etop == 0:                                                   # all zero, or the model wholly outside the frame: exact zeros
            assert not got["bins"][i].any() and not got["energy"][i].any()
        assert abs(float(got["energy"][i][6]) - float((np.abs(got["bins"][i]) ** 2).sum())) <= 1e-12 * max(etop, 1.0)      # trial 6 is the given start
    print(f"ft4 sub probe worst: model {worst[0]:.3e}, bins {worst[1]:.3e}, energy {worst[2]:.3e}")
    assert worst[0] <= MODEL_BOUND and worst[1] <= BINS_BOUND and worst[2] <= ENERGY_BOUND
    again = handle.ft4_sub_probe(audio, frame[:1], cases.subsig_array(sigs[:1]))       # a signal alone: the same bits
    assert again["bins"].tobytes() == got["bins"][:1].tobytes() and again["energy"].tobytes() == got["energy"][:1].tobytes()


# ----------------------------------------------------------------------------- 2. refine decisions
def test_refine_decisions_are_the_twins(handle):
    audio, frame, sigs, truth = cases.probe_cases()
    _, _, en, want = cases.probe_twin()
    # the fixture first: every case with energy decides by a margin of at least 20 x the energy bound (a case of exact zeros is
    # decided by the order of the trials alone: the first one)
    for i, e in enumerate(en):
        gap = cases.energy_gap(e)
        print(f"ft4 sub refine {i}: twin start {want[i]} (given {sigs[i]['start']}, true {truth[i]}), gap {gap:.3e}")
        assert gap >= 20.0 * ENERGY_BOUND or not e.any()
        if truth[i] is not None and cases.PROBE[i][3] >= -5.0:
            assert abs(want[i] - truth[i]) <= 2
    got = [None] * len(sigs)
    per_frame = [[i for i in range(len(sigs)) if frame[i] == f] for f in range(3)]
    for r in range(max(len(p) for p in per_frame)):                         # one signal per frame and call, each on the untouched frames
        lists = [[(sigs[p[r]]["start"], sigs[p[r]]["fq"], sigs[p[r]]["tones"])] if r < len(p) else [] for p in per_frame]
        d = _device(audio)
        arr, cnt, _ = handle.ft4_subtract(d.data_ptr(), 3, lists, refine=1)
        for f, p in enumerate(per_frame):
            if r < len(p):
                got[p[r]] = int(arr[f, 0]["start"])
    assert got == want
    e_gpu = handle.ft4_sub_probe(audio, frame, cases.subsig_array(sigs))["energy"]
    assert [s["start"] + ft4.SUB_SHIFTS[int(np.argmax(e))] for s, e in zip(sigs, e_gpu)] == want


# ----------------------------------------------------------------------------- 3. residual
def test_residual_of_a_batch(handle):
    audio, sigs = cases.residual_cases()
    lists = [[(s["start"], s["fq"], s["tones"]) for s in fs] for fs in sigs]
    d = _device(audio)
    arr, cnt, res = handle.ft4_subtract(d.data_ptr(), 3, lists, refine=1, return_float=True)
    i16 = d.cpu().numpy()
    assert cnt.tolist() == [4, 4, 4] and res.dtype == np.float32 and res.shape == audio.shape
    worst = worst_rms = 0.0
    for f in range(3):
        starts = [int(s) for s in arr[f]["start"]]
        want = cases.twin_residual(audio[f], sigs[f], starts)
        rms = float(np.sqrt((audio[f].astype(np.float64) ** 2).mean()))
        err = float(np.abs(res[f] - want).max())
        print(f"ft4 sub residual frame {f}: starts {[a - s['start'] for a, s in zip(starts, sigs[f])]} from the given, max error {err:.3e} counts "
              f"= {err / rms:.3e} of the RMS {rms:.0f}; energy {float((res[f].astype(np.float64) ** 2).sum() / (audio[f].astype(np.float64) ** 2).sum()):.3f} of the frame's")
        worst, worst_rms = max(worst, err), max(worst_rms, err / rms)
        for k, ((f0, start, snr, _), st) in enumerate(zip(cases.RESIDUAL[f], starts)):
            if snr >= 0.0 and (f, k) not in cases.RESIDUAL_PAIRS:               # alone and at 0 dB or above: within 3 samples under noise
                assert abs(st - start) <= 3
    print(f"ft4 sub residual worst: {worst:.3e} counts, {worst_rms:.3e} of the RMS")
    assert worst <= RESIDUAL_BOUND and worst_rms <= 1e-4
    # list order matters: the pair of frame 1 in the other order leaves something else
    f = 1
    swapped = cases.twin_residual(audio[f], [sigs[f][1], sigs[f][0]] + sigs[f][2:], [int(arr[f, 1]["start"]), int(arr[f, 0]["start"])] + [int(s) for s in arr[f, 2:]["start"]])
    assert float(np.abs(res[f] - swapped).max()) > 100.0 * RESIDUAL_BOUND
    assert np.array_equal(i16, np.clip(np.rint(res), -32768, 32767).astype(np.int16))
    # a second run: the same bytes
    d2 = _device(audio)
    arr2, _, res2 = handle.ft4_subtract(d2.data_ptr(), 3, lists, refine=1, return_float=True)
    assert res2.tobytes() == res.tobytes() and arr2.tobytes() == arr.tobytes() and d2.cpu().numpy().tobytes() == i16.tobytes()
    # a frame alone: the bytes it has in the batch
    d1 = _device(audio[1:2])
    arr1, _, res1 = handle.ft4_subtract(d1.data_ptr(), 1, lists[1:2], refine=1, return_float=True)
    assert res1[0].tobytes() == res[1].tobytes() and arr1[0].tobytes() == arr[1].tobytes() and d1.cpu().numpy()[0].tobytes() == i16[1].tobytes()
    # a frame with count 0 keeps its bytes
    d0 = _device(audio)
    _, cnt0, res0 = handle.ft4_subtract(d0.data_ptr(), 3, [lists[0], [], lists[2]], refine=1, return_float=True)
    out0 = d0.cpu().numpy()
    assert cnt0.tolist() == [4, 0, 4] and out0[1].tobytes() == audio[1].tobytes() and np.array_equal(res0[1], audio[1].astype(np.float32))
    assert out0[0].tobytes() == i16[0].tobytes() and out0[2].tobytes() == i16[2].tobytes()
    # refine 0 keeps the given starts
    arr_0, _, _ = handle.ft4_subtract(_device(audio).data_ptr(), 3, lists, refine=0)
    assert [int(s) for s in arr_0[0]["start"]] == [s["start"] for s in sigs[0]]


# ----------------------------------------------------------------------------- 4. end to end
def _texts(msgs):
    return [" ".join(x for x in m["msg_tuple"] if x) for m in msgs]


def _same(a, b):
    drop = lambda d: {k: v for k, v in d.items() if k != "decode_completed"}
    return [drop(x) for x in a] == [drop(x) for x in b]


@pytest.fixture(scope="module")
def crowded_out():
    """the crowded frames through receivers of 1, 2 and 3 passes -> {passes: per-frame dict lists}"""
    audio = np.stack([cases.crowded(i)[0] for i in cases.CROWDED])
    out = {}
    for p in (1, 2, 3):
        r = Receiver("", None, max_frames=3, max_cands=60, ft4_passes=p)
        try:
            out[p] = r.decode_frames_ft4(audio)
        finally:
            r.close()
    return out


def test_end_to_end_two_passes(crowded_out):
    one, two, three = crowded_out[1], crowded_out[2], crowded_out[3]
    tot = {1: 0, 2: 0, 3: 0}
    for f, index in enumerate(cases.CROWDED):
        planted = {t["msg"] for t in cases.crowded(index)[1]}
        t1, t2, t3 = _texts(one[f]), _texts(two[f]), _texts(three[f])
        n1, n2, n3 = (sum(t in planted for t in tt) for tt in (t1, t2, t3))
        print(f"ft4 passes frame {index}: {n1} / {n2} / {n3} true decodes of 16 with 1 / 2 / 3 passes; unplanted {[t for t in t3 if t not in planted]}")
        assert n2 >= n1 and n3 >= n2                                         # no frame with fewer
        assert _same(two[f][:len(one[f])], one[f]) and _same(three[f][:len(two[f])], two[f])      # the earlier passes' dicts, unchanged, at the head
        for d in two[f][len(one[f]):] + three[f][len(one[f]):]:
            assert "_SUB" in d["decode_notes"] and d["mode"] == "FT4"
        assert all("_SUB" not in d["decode_notes"] for d in one[f])
        assert len(set(t2)) == len(t2) and len(set(t3)) == len(t3)
        assert {t for t in t3 if t not in planted} <= {t for t in t1 if t not in planted}       # nothing unplanted that one pass does not show
        for k, n in zip((1, 2, 3), (n1, n2, n3)):
            tot[k] += n
    print(f"ft4 passes total: {tot[1]} / {tot[2]} / {tot[3]} of 48 (the twin: {cases.TWIN_PASS1} -> {cases.TWIN_TOTAL})")
    assert tot[2] > tot[1] and tot[2] >= cases.TWIN_TOTAL - 2 and tot[3] >= tot[2]


def test_end_to_end_callbacks_and_records():
    audio = np.stack([cases.crowded(i)[0] for i in cases.CROWDED[:2]])
    seen = []
    r = Receiver("", seen.append, max_frames=2, max_cands=60, ft4_passes=2)
    try:
        out, rec, cnt = r.decode_frames_ft4(audio, return_records=True)
        assert sum(len(o) for o in out) == len(seen) and all(any(d is s for s in seen) for o in out for d in o)      # once per message
        for f in range(2):
            assert [id(d) for d in seen if any(d is x for x in out[f])] == [id(d) for d in out[f]]                  # in the final order
        assert rec.shape == (2, 60) and rec.dtype == _lib.RECORD_DTYPE and cnt.shape == (2,)
        one = decode_frames_ft4(audio[:1], max_cands=60, ft4_passes=2)                                              # the module-level entry
        assert _texts(one[0]) == _texts(out[0]) and _texts(r.decode_frame_ft4(audio[0])) == _texts(out[0])
    finally:
        r.close()


# ----------------------------------------------------------------------------- 5. with msg_types
def test_contest_message_under_a_strong_one():
    x, strong, weak = cases.hidden_frame()
    one = decode_frames_ft4(x[None], msg_types="all")[0]
    two = decode_frames_ft4(x[None], msg_types="all", ft4_passes=2)[0]
    print("ft4 passes hidden:", _texts(one), "->", [(t, d["decode_notes"]) for t, d in zip(_texts(two), two)])
    assert _texts(one) == ["CQ K1ABC FN42"]
    assert _texts(two) == ["CQ K1ABC FN42", cases.HIDDEN_TEXT]
    assert two[1]["msg_type"] == "3" and "_SUB" in two[1]["decode_notes"] and two[1]["mode"] == "FT4" and _same(two[:1], one)
    assert abs(two[1]["fHz"] - 1006.0) <= 2.7 and abs(two[1]["tsec"] - 0.6) <= 0.02


# ----------------------------------------------------------------------------- 6. nothing else moved
def test_one_pass_is_todays():
    audio = np.stack([ft4_cases.six(i)[0] for i in ft4_cases.SIX])
    a, b = Receiver("", None, max_frames=3), Receiver("", None, max_frames=3, ft4_passes=1)
    try:
        ra, rb = a.decode_frames_ft4(audio, return_records=True), b.decode_frames_ft4(audio, return_records=True)
        assert all(_same(x, y) for x, y in zip(ra[0], rb[0])) and sum(len(x) for x in ra[0]) >= 18
        assert ra[1].tobytes() == rb[1].tobytes() and ra[2].tobytes() == rb[2].tobytes()
        assert b._handle(3).ft4_sub_info()["workspace_bytes"] == 0          # one pass: nothing of the subtraction is allocated
    finally:
        a.close(); b.close()


def test_ft8_after_two_passes_is_byte_identical_and_no_workspace_without_subtraction():
    audio8 = synth.make_frame(7, n_signals=12, snr_range=(-12.0, 5.0))
    fresh, used = _lib.Handle(max_frames=1), _lib.Handle(max_frames=1)
    try:
        assert used.ft4_staging_ptr() == 0 and used.ft4_sub_info()["workspace_bytes"] == 0
        x = ft4_cases.six()[0]
        res = used.ft4_decode(x)
        before = used.ft4_info()["workspace_bytes"]
        assert used.ft4_sub_info()["workspace_bytes"] == 0 and used.ft4_staging_ptr() != 0          # decoding FT4 allocates nothing of the subtraction
        sg = _lib.ft4_subtraction_list(res[0], res[1])
        assert int(sg[1][0]) >= 6
        used.ft4_subtract(used.ft4_staging_ptr(), 1, sg, refine=1)
        used.ft4_enqueue(used.ft4_staging_ptr(), 1)
        rec2, cnt2 = used.fetch(1)[:2]
        assert (rec2[0, :int(cnt2[0])]["status"] == _lib.ST_DECODED).sum() == 0         # six clean signals: nothing is left to decode
        assert used.ft4_sub_info()["workspace_bytes"] > 90000 * 4 and used.ft4_info()["workspace_bytes"] == before
        assert fresh.ft4_sub_info()["workspace_bytes"] == 0
        a, b = fresh.decode_batch(audio8), used.decode_batch(audio8)
        n, ne = int(a[1][0]), int(a[3][0])
        assert n > 0 and ne > 0 and int(b[1][0]) == n and int(b[3][0]) == ne and a[0][0, :n].tobytes() == b[0][0, :n].tobytes()
        key = lambda ev: sorted(e.tobytes() for e in ev)
        assert key(a[2][0, :ne]) == key(b[2][0, :ne])
    finally:
        fresh.close(); used.close()


def test_refusals(handle):
    r = Receiver("", None, max_frames=1, ft4_passes=2)
    try:
        with pytest.raises(_lib.Ft8rxError, match=r"passes > 1"):
            r.decode_frames_ft4(ft4_cases.zero_frame(), passes=2)
        assert r.decode_frames_ft4(ft4_cases.zero_frame()) == [[]]
    finally:
        r.close()
    for bad in (0, 4, "x", True, 2.0):
        with pytest.raises(_lib.Ft8rxError, match="ft4_passes"):
            Receiver("", None, max_frames=1, ft4_passes=bad)
    for kw, name in ((dict(my_call="K1ABC"), "my_call / dx_call"), (dict(recall=True), "recall"), (dict(weak=True), "weak=True"),
                     (dict(reports=True), "reports=True"), (dict(float_frames=True), "float_frames=True")):
        r = Receiver("", None, max_frames=1, ft4_passes=2, **kw)
        try:
            with pytest.raises(_lib.Ft8rxError, match=r"FT4 decoding \(decode_frames_ft4\) is not supported together with " + name.replace("(", r"\(")):
                r.decode_frames_ft4(ft4_cases.zero_frame())
        finally:
            r.close()
    audio, _, sigs, _ = cases.probe_cases()
    one = [[(sigs[0]["start"], sigs[0]["fq"], sigs[0]["tones"])]]
    d = _device(audio[:1])
    with pytest.raises(_lib.Ft8rxError, match="refine 2"):
        handle.ft4_subtract(d.data_ptr(), 1, one, refine=2)
    with pytest.raises(_lib.Ft8rxError, match="out of range"):
        handle.ft4_subtract(d.data_ptr(), 1, [[(0, 4608, sigs[0]["tones"])]])
    with pytest.raises(_lib.Ft8rxError, match="out of range"):
        handle.ft4_subtract(d.data_ptr(), 1, [[(0, 100, [4] * 105)]])
    with pytest.raises(_lib.Ft8rxError, match="out of range"):
        handle.ft4_sub_probe(audio[:1], [1], cases.subsig_array(sigs[:1]))
    assert d.cpu().numpy().tobytes() == audio[:1].tobytes()                 # a refused call touches nothing
