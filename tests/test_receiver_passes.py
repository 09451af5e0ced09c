"""CPU-only tests of Receiver's orchestration: which calls every entry (decode_frames, decode_frames_arrays, decode_stream, poll at
12 kHz and with wide input) makes on its handle, in which order and with which arguments, and what it returns.  _lib.Handle is replaced
by a recording stand-in whose decode_batch / fetch hand out the oracle's dense results of golden frames; the native host message layer
(package_batch*, merge_messages, subtraction_list) is the real one, so the messages are the goldens' own.  The traces and counts are
literals: they are what the receiver did before its passes were written once, and what it must keep doing."""
import collections

import numpy as np
import pytest

from conftest import load_golden
from helpers import oracle_frame, records_from_oracle
from pyft8_amd import _lib, ddc, ddc_rat, ddc_wide, receiver

NAMES = ("test_08", "test_09")
N_MSGS = {"test_08": 21, "test_09": 20}
STAGING = 0x5A5A00
_dense_cache = {}


def dense(names):
    """The oracle's dense results of the golden frames `names` as one batch (test_host_layer._dense_goldens)"""
    for nm in names:
        if nm not in _dense_cache:
            rec, n, ev, nev = records_from_oracle(oracle_frame(load_golden(nm)[0]))
            e = np.zeros(_lib.EVENT_CAP, _lib.EVENT_DTYPE)
            e[:len(ev)] = ev[:_lib.EVENT_CAP]
            _dense_cache[nm] = (rec, n, e, nev)
    r = [_dense_cache[nm] for nm in names]
    return (np.stack([x[0] for x in r]), np.array([x[1] for x in r], np.int32), np.stack([x[2] for x in r]),
            np.array([x[3] for x in r], np.int32))


def texts(name):
    return [" ".join(m["msg_tuple"]) for m in load_golden(name)[2]["messages"]]


def got(dicts):
    return [" ".join(d["msg_tuple"]) for d in dicts]


def audio(n=2):
    return np.stack([load_golden(nm)[0] for nm in NAMES[:n]])


class Tape:
    """What the stand-in handles of one test share: the calls made (`calls`), the packaging calls (`pkg`), the results to hand out"""
    def __init__(self):
        self.calls, self.pkg, self.results, self.handles = [], [], collections.deque(), []
        self.blank_params = self.recall_entries = None
        self.tables = []                     # the table= of every packaging call

    def push(self, *batches):
        """queue one dense result per batch; a batch is a tuple of golden names"""
        for names in batches:
            self.results.append(dense(names))

    def take(self):
        calls, self.calls = self.calls, []
        return calls

    def take_pkg(self):
        pkg, self.pkg = self.pkg, []
        return pkg


def stand_in(tape):
    class Handle:
        def __init__(self, cfg=None, device=0, max_frames=1):
            self.cfg, self.max_frames = cfg, int(max_frames)
            tape.handles.append(self)

        def _result(self, B):
            res = tape.results.popleft()
            assert len(res[1]) == B
            return res

        def set_ladder_mode(self, mode):
            pass

        def close(self):
            pass

        def decode_batch(self, audio):
            assert audio.dtype == np.int16 and audio.shape[1:] == (_lib.NSAMP,)
            tape.calls.append(f"decode_batch({len(audio)})")
            return self._result(len(audio))

        def staging_ptr(self):
            tape.calls.append("staging_ptr")
            return STAGING

        def enqueue(self, ptr, B):
            assert ptr == STAGING
            tape.calls.append(f"enqueue({B})")

        def fetch(self, B):
            tape.calls.append(f"fetch({B})")
            return self._result(B)

        def fetch_reports(self, B):
            tape.calls.append(f"fetch_reports({B})")
            return np.zeros((B, self.cfg.max_cands), _lib.REPORT_DTYPE)

        def set_recall(self, entries):
            tape.recall_entries = entries
            tape.calls.append(f"set_recall({[len(e) for e in entries]})")

        def fetch_recall(self, B):
            tape.calls.append(f"fetch_recall({B})")
            return np.zeros((B, _lib.RECALL_MAX), _lib.RECORD_DTYPE), np.zeros(B, np.int32)

        def blank_host(self, audio, *params):
            tape.blank_params = params
            tape.calls.append(f"blank_host({len(audio)})")
            return np.zeros((len(audio), 4), np.int32)

        def blank(self, ptr, B, *params):
            assert ptr is None
            tape.blank_params = params
            tape.calls.append(f"blank({B})")
            return np.zeros((B, 4), np.int32)

        def subtract(self, ptr, B, sigs, refine=False):
            assert ptr == STAGING and sigs[0].dtype == _lib.SUBSIG_DTYPE
            tape.calls.append(f"subtract({B},{sigs[1].tolist()},refine={refine})")

        def set_search_mask(self, mask):
            tape.calls.append("set_search_mask(None)" if mask is None else f"set_search_mask({mask.shape})")

        def ddc(self, arr, kind, rate, src, dials):
            tape.calls.append(f"ddc({arr.shape},{arr.dtype},{kind},{rate},{list(src)},{list(dials)})")

        def ddc_wide(self, arr, kind, rate, dials):
            tape.calls.append(f"ddc_wide({arr.shape},{arr.dtype},{kind},{rate},{list(dials)})")

        def ddc_rat(self, arr, kind, rate, dials):
            tape.calls.append(f"ddc_rat({arr.shape},{arr.dtype},{kind},{rate},{list(dials)})")

        def ddc_stream_frame(self, m_first, n_have):
            tape.calls.append(f"ddc_stream_frame({m_first},{n_have})")

        # the streams of the live wide input: what was opened, and per push the shape, dtype and first value of the samples
        def _open(self, name, kind, rate, *rest):
            self.rate, self.n_in = rate, 0
            tape.calls.append(f"{name}({kind},{rate},{','.join(str(list(x) if isinstance(x, (list, tuple)) else x) for x in rest)})")
            return np.zeros(len(rest[-1]))

        def _push(self, name, a, n):
            tape.calls.append(f"{name}({a.shape},{a.dtype},{a.reshape(-1)[0]})")
            self.n_in += n
            return max(0, self.n_in * 12000 // self.rate - 1200) // 1008 * 1008

        def ddc_stream_open(self, kind, rate, n_streams, src, dials):
            return self._open("ddc_stream_open", kind, rate, n_streams, src, dials)

        def ddc_wide_stream_open(self, kind, rate, dials):
            return self._open("ddc_wide_stream_open", kind, rate, dials)

        def ddc_rat_stream_open(self, kind, rate, dials):
            return self._open("ddc_rat_stream_open", kind, rate, dials)

        def ddc_stream_push(self, a):
            return self._push("ddc_stream_push", a, a.shape[1])

        def ddc_wide_stream_push(self, a):
            return self._push("ddc_wide_stream_push", a, a.shape[0])

        def ddc_rat_stream_push(self, a):
            return self._push("ddc_rat_stream_push", a, a.shape[0])

    return Handle


@pytest.fixture
def tape(monkeypatch):
    t = Tape()
    monkeypatch.setattr(_lib, "Handle", stand_in(t))

    def recorded(name):
        fn = getattr(_lib, name)

        def wrapper(*a, **kw):
            res = fn(*a, **kw)
            what = {k: ("table" if k == "table" else v) for k, v in kw.items()}
            if name == "package_batch_ext":
                what["mask"] = a[4]
            if name == "merge_messages":
                what["tag"] = a[4]
            else:
                what["rows"] = "ext" if res[0].dtype == _lib.MESSAGE_EXT_DTYPE else "plain"
                t.tables.append(kw.get("table"))
            t.pkg.append((name, what))
            return res
        monkeypatch.setattr(_lib, name, wrapper)
    for name in ("package_batch", "package_batch_ext", "package_batch_recall", "merge_messages"):
        recorded(name)
    return t


def rx_of(cb=None, **kw):
    kw.setdefault("max_frames", 2)
    return receiver.Receiver("", cb.append if cb is not None else None, autostart=False, time_source=lambda: 15000.0, **kw)


PLAIN = ["decode_batch(2)"]
STAGED = ["staging_ptr", "enqueue(2)", "fetch(2)"]
PKG1 = ("package_batch", {"rows": "plain"})


# ---- decode_frames
def test_decode_frames_plain(tape):
    cb = []
    rx = rx_of(cb)
    tape.push(NAMES)
    out = rx.decode_frames(audio(), cyclestart_strings=["250101_000000", "250101_000015"])
    assert tape.take() == PLAIN and tape.take_pkg() == [PKG1]
    assert [got(o) for o in out] == [texts(nm) for nm in NAMES] and [len(o) for o in out] == [21, 20]
    assert [d["cyclestart_string"] for d in out[1]] == ["250101_000015"] * 20 and out[0][0]["cyclestart_string"] == "250101_000000"
    assert all("recall" not in d and "report" not in d and "channel" not in d and d["band"] is None for o in out for d in o)
    assert len(cb) == 41 and all(a is b for a, b in zip(cb, out[0] + out[1]))
    assert len(tape.handles) == 1 and rx.blanker_stats is None
    # one frame more than the handle holds: a new handle; the module-level entry and decode_frame go the same way
    tape.push(NAMES + NAMES[:1])
    assert [len(o) for o in rx.decode_frames(np.concatenate([audio(), audio(1)]))] == [21, 20, 21]
    assert tape.take() == ["decode_batch(3)"] and len(tape.handles) == 2 and tape.handles[1].max_frames == 3
    tape.push(NAMES[1:], NAMES)
    assert got(rx.decode_frame(audio()[1], "250101_000030")) == texts("test_09")
    assert [got(o) for o in receiver.decode_frames(audio())] == [texts(nm) for nm in NAMES]
    assert tape.take() == ["decode_batch(1)", "decode_batch(2)"]


def test_decode_frames_empty_batch(tape):
    rx = rx_of()
    assert rx.decode_frames(np.zeros((0, _lib.NSAMP), np.int16)) == []
    out, rec, cnt = rx.decode_frames(np.zeros((0, _lib.NSAMP), np.int16), return_records=True)
    assert out == [] and rec.shape == (0, 200) and rec.dtype == _lib.RECORD_DTYPE and cnt.shape == (0,)
    with pytest.raises(_lib.Ft8rxError, match="empty batch"):
        rx.decode_frames_arrays(np.zeros((0, _lib.NSAMP), np.int16))
    with pytest.raises(_lib.Ft8rxError, match="one list of earlier messages per frame"):
        rx.decode_frames(audio(), recall=[[]])
    with pytest.raises(_lib.Ft8rxError, match="research must be"):
        rx.decode_frames(audio(), research="wide")
    assert tape.take() == [] and tape.take_pkg() == []


def test_decode_frames_two_passes_with_the_blanker(tape):
    """The second batch is the two results swapped: every text of the other frame that this frame lacks is new."""
    cb = []
    rx = rx_of(cb, noise_blanker=3.0)
    tape.push(NAMES, NAMES[::-1])
    out = rx.decode_frames(audio(), passes=2)
    assert tape.take() == ["blank_host(2)"] + STAGED + ["staging_ptr", "subtract(2,[18, 19],refine=2)"] + STAGED
    assert tape.take_pkg() == [PKG1, PKG1]                           # the later passes: plain package_batch, default threads
    assert tape.blank_params == (768, 6, 6) and rx.blanker_stats.shape == (2, 4)
    assert [len(o) for o in out] == [21 + 20, 20 + 21]
    assert got(out[0]) == texts("test_08") + texts("test_09") and got(out[1]) == texts("test_09") + texts("test_08")
    assert [d["decode_notes"].endswith("_SUB") for d in out[0]] == [False] * 21 + [True] * 20
    assert [d["decode_notes"].endswith("_SUB") for d in out[1]] == [False] * 20 + [True] * 21
    # callbacks: pass 1 frame by frame, then pass 2 frame by frame
    order = out[0][:21] + out[1][:20] + out[0][21:] + out[1][20:]
    assert len(cb) == 82 and all(a is b for a, b in zip(cb, order))


def test_decode_frames_third_pass_stops_on_an_empty_list(tape):
    """Pass 2 brings the same messages again: nothing is new, the loop goes on with an empty subtraction list and stops there."""
    rx = rx_of()
    tape.push(NAMES, NAMES)
    out, rec, cnt = rx.decode_frames(audio(), passes=3, return_records=True)
    assert tape.take() == PLAIN + ["staging_ptr", "subtract(2,[18, 19],refine=2)"] + STAGED
    assert [got(o) for o in out] == [texts(nm) for nm in NAMES] and not tape.results


def test_decode_frames_three_passes(tape):
    """Only the fresh messages of a pass are subtracted before the next one."""
    rx = rx_of()
    tape.push(NAMES, NAMES[::-1], ("test_08", "test_08"))
    out = rx.decode_frames(audio(), passes=3)
    assert tape.take() == PLAIN + ["staging_ptr", "subtract(2,[18, 19],refine=2)"] + STAGED + \
        ["staging_ptr", "subtract(2,[19, 18],refine=2)"] + STAGED
    assert tape.take_pkg() == [PKG1] * 3
    assert [len(o) for o in out] == [41, 41]


def test_decode_frames_local_research(tape):
    """research="local": the mask is set for the residual decode and cleared behind it; one sweep only, whatever `passes` says."""
    rx = rx_of()
    tape.push(NAMES, NAMES[::-1])
    out = rx.decode_frames(audio(), passes=3, research="local")
    assert tape.take() == PLAIN + ["staging_ptr", "subtract(2,[18, 19],refine=2)", "set_search_mask((2, 928))"] + STAGED + \
        ["set_search_mask(None)"]
    assert [len(o) for o in out] == [41, 41]

    class Boom(RuntimeError):
        pass

    def failing_fetch(B):
        raise Boom
    tape.push(NAMES)
    h = tape.handles[-1]
    h.fetch = failing_fetch
    with pytest.raises(Boom):
        rx.decode_frames(audio(), passes=2, research="local")
    assert tape.take()[-2:] == ["enqueue(2)", "set_search_mask(None)"]          # cleared in `finally`


def test_decode_frames_sub_pass_osd(tape):
    rx = rx_of()
    tape.push(NAMES, NAMES[::-1], NAMES, NAMES[::-1])
    with_osd = rx.decode_frames(audio(), passes=2)
    without = rx.decode_frames(audio(), passes=2, sub_pass_osd=False)
    for f in range(2):
        n1 = N_MSGS[NAMES[f]]
        assert got(without[f][:n1]) == got(with_osd[f][:n1])                      # the first pass keeps its OSD decodes
        assert got(without[f][n1:]) == [" ".join(d["msg_tuple"]) for d in with_osd[f][n1:] if "OSD" not in d["decode_notes"]]
    assert [len(o) for o in without] == [39, 40]


def test_decode_frames_return_records(tape):
    """decode_frames hands back the records of the LAST pass that ran, decode_frames_arrays those of the FIRST."""
    rx = rx_of()
    first, second = dense(NAMES), dense(NAMES[::-1])
    tape.push(NAMES)
    out, rec, cnt = rx.decode_frames(audio(), return_records=True)
    assert rec.tobytes() == first[0].tobytes() and cnt.tolist() == first[1].tolist()
    tape.push(NAMES, NAMES[::-1])
    out, rec, cnt = rx.decode_frames(audio(), return_records=True, passes=2)
    assert rec.tobytes() == second[0].tobytes() and [len(o) for o in out] == [41, 41]
    tape.push(NAMES, NAMES[::-1])
    msgs, mcnt, rec, cnt = rx.decode_frames_arrays(audio(), passes=2)
    assert rec.tobytes() == first[0].tobytes() and cnt.tolist() == first[1].tolist()


def test_decode_frames_recall(tape):
    rx = rx_of()
    tape.push(NAMES)
    prev = rx.decode_frames(audio())
    tape.take(), tape.take_pkg()
    tape.push(NAMES)
    out = rx.decode_frames(audio(), recall=[prev[0], None])
    assert tape.take() == ["set_recall([19, 0])"] + PLAIN + ["fetch_recall(2)"]
    assert tape.take_pkg() == [("package_batch_recall", {"rows": "plain"})]
    assert [got(o) for o in out] == [texts(nm) for nm in NAMES] and all(d["recall"] is False for o in out for d in o)
    # a receiver with recall on and no list: empty entries are still set
    rx = rx_of(recall=True, noise_blanker=True)
    tape.push(NAMES)
    out = rx.decode_frames(audio())
    assert tape.take() == ["set_recall([0, 0])", "blank_host(2)"] + STAGED + ["fetch_recall(2)"]
    assert tape.blank_params == (2048, 6, 6) and all("recall" in d for o in out for d in o)
    with pytest.raises(_lib.Ft8rxError, match="passes > 1 .* is not supported together with recall"):
        rx.decode_frames(audio(), passes=2)
    assert tape.take() == []


def test_decode_frames_reports_and_message_types(tape):
    rx = rx_of(reports=True)
    tape.push(NAMES)
    out = rx.decode_frames(audio())
    assert tape.take() == PLAIN + ["fetch_reports(2)"] and tape.take_pkg() == [PKG1]
    assert [len(o) for o in out] == [21, 20] and all(d["report"] is None for o in out for d in o)
    rx = rx_of(msg_types="all", reports=True, noise_blanker=True)
    tape.push(NAMES)
    out = rx.decode_frames(audio())
    assert tape.take() == ["blank_host(2)"] + STAGED + ["fetch_reports(2)"]
    assert tape.take_pkg() == [("package_batch_ext", {"mask": _lib.MT_ALL, "rows": "ext"})]
    assert [got(o) for o in out] == [texts(nm) for nm in NAMES]


# ---- decode_frames_arrays
def test_decode_frames_arrays(tape):
    rx = rx_of()
    tape.push(NAMES)
    msgs, mcnt, rec, cnt = rx.decode_frames_arrays(audio(), n_threads=3)
    assert tape.take() == PLAIN and tape.take_pkg() == [("package_batch", {"n_threads": 3, "rows": "plain"})]
    assert msgs.dtype == _lib.MESSAGE_DTYPE and mcnt.tolist() == [21, 20] and not msgs["pad"][:, :, 0].any()
    rx = rx_of(noise_blanker=3.0)
    tape.push(NAMES, NAMES[::-1])
    msgs, mcnt, rec, cnt = rx.decode_frames_arrays(audio(), n_threads=2, passes=2)
    assert tape.take() == ["blank_host(2)"] + STAGED + ["staging_ptr", "subtract(2,[18, 19],refine=2)"] + STAGED
    p = ("package_batch", {"n_threads": 2, "rows": "plain"})
    assert tape.take_pkg() == [p, p, ("merge_messages", {"drop_osd": False, "tag": 1})]
    assert mcnt.tolist() == [41, 41] and rx.blanker_stats.shape == (2, 4)
    assert msgs["pad"][0, :41, 0].tolist() == [0] * 21 + [1] * 20 and msgs["pad"][1, :41, 0].tolist() == [0] * 20 + [1] * 21
    tape.push(NAMES, NAMES[::-1], ("test_08", "test_08"))
    msgs, mcnt, rec, cnt = rx.decode_frames_arrays(audio(), passes=3, sub_pass_osd=False, research="local")
    assert tape.take() == ["blank_host(2)"] + STAGED + ["staging_ptr", "subtract(2,[18, 19],refine=2)", "set_search_mask((2, 928))"] + \
        STAGED + ["set_search_mask(None)"]
    assert mcnt.tolist() == [39, 40] and tape.take_pkg()[-1] == ("merge_messages", {"drop_osd": True, "tag": 1})
    tape.results.clear()
    tape.push(NAMES, NAMES[::-1], ("test_08", "test_08"))
    msgs, mcnt, rec, cnt = rx.decode_frames_arrays(audio(), passes=3)
    assert [c for c in tape.take() if c.startswith("subtract")] == ["subtract(2,[18, 19],refine=2)", "subtract(2,[19, 18],refine=2)"]
    assert [x[1].get("tag") for x in tape.take_pkg() if x[0] == "merge_messages"] == [1, 2] and mcnt.tolist() == [41, 41]
    tape.push(NAMES, NAMES)                                      # nothing new in pass 2: the empty list stops pass 3
    msgs, mcnt, rec, cnt = rx.decode_frames_arrays(audio(), passes=3)
    assert mcnt.tolist() == [21, 20] and len(tape.take()) == 9 and not tape.results


@pytest.mark.parametrize("kw, name", [(dict(msg_types="all"), "msg_types != 0"), (dict(recall=True), "recall"),
                                      (dict(reports=True), "reports=True")])
def test_decode_frames_arrays_refusals(tape, kw, name):
    rx = rx_of(**kw)
    with pytest.raises(_lib.Ft8rxError) as e:
        rx.decode_frames_arrays(audio())
    assert str(e.value) == f"decode_frames_arrays is not supported together with {name}: its _lib.MESSAGE_DTYPE rows have no place " \
                           "for them; use decode_frames"
    assert tape.take() == []
    with pytest.raises(_lib.Ft8rxError, match="research must be"):
        rx.decode_frames_arrays(audio(), research="none")


# ---- decode_stream
def test_decode_stream_front_ends(tape):
    rx = rx_of(noise_blanker=True)
    pairs = np.ones((1000, 2), np.int16)
    tape.push(NAMES)
    out = rx.decode_stream(pairs, 48000, iq=True, dial_offsets_hz=(-1000, 2000), bands=("a", "b"))
    assert tape.take() == [f"ddc((1, 1000, 2),int16,{ddc.IQ_I16},48000,[0, 0],[-1000.0, 2000.0])", "blank(2)"] + STAGED
    assert [got(o) for o in out] == [texts(nm) for nm in NAMES]
    assert [{d["band"] for d in o} for o in out] == [{"a"}, {"b"}] and all("channel" not in d for o in out for d in o)
    # two real float streams, one channel each; complex input; an explicit src
    rx = rx_of()
    tape.push(NAMES, NAMES, NAMES)
    rx.decode_stream(np.zeros((2, 500), np.float64), 24000, dial_offsets_hz=(0.0, 0.0))
    rx.decode_stream(np.zeros(500, np.complex128), 12000, iq=True, dial_offsets_hz=(0.0, 100.0), passes=1)
    rx.decode_stream(np.zeros((3, 500), np.int32), 192000, dial_offsets_hz=(0.0, 0.0), src=(2, 1))
    assert tape.take() == [f"ddc((2, 500),float32,{ddc.REAL_F32},24000,[0, 1],[0.0, 0.0])"] + STAGED + \
        [f"ddc((1, 500, 2),float32,{ddc.IQ_F32},12000,[0, 0],[0.0, 100.0])"] + STAGED + \
        [f"ddc((3, 500),int16,{ddc.REAL_I16},192000,[2, 1],[0.0, 0.0])"] + STAGED
    # a wide rate and a resampled rate: ONE stream, [n(, 2)]
    tape.push(NAMES, NAMES[::-1], NAMES[:1], NAMES[:1])
    out = rx.decode_stream(np.full((1, 700, 2), 128, np.uint8), 240000, iq=True, dial_offsets_hz=(7074000.0, 7076000.0), src=[0, 0],
                           passes=2, resample=True)
    assert tape.take() == [f"ddc_wide((700, 2),uint8,{ddc_wide.IQ_U8},240000,[7074000.0, 7076000.0])"] + STAGED + \
        ["staging_ptr", "subtract(2,[18, 19],refine=2)"] + STAGED
    assert [len(o) for o in out] == [41, 41]
    rx.decode_stream(np.zeros(441, np.int16), 44100, resample=True)
    rx.decode_stream(np.zeros(441, np.complex64), 2048000, iq=True, resample=True, dial_offsets_hz=[5.0])
    assert tape.take() == [f"ddc_rat((441,),int16,{ddc_rat.REAL_I16},44100,[0.0])", "staging_ptr", "enqueue(1)", "fetch(1)",
                           f"ddc_rat((441, 2),float32,{ddc_rat.IQ_F32},2048000,[5.0])", "staging_ptr", "enqueue(1)", "fetch(1)"]


def test_decode_stream_refusals(tape):
    rx = rx_of()
    E = _lib.Ft8rxError
    with pytest.raises(E, match="^samples are complex: pass iq=True$"):
        rx.decode_stream(np.zeros(500, np.complex64), 48000)
    with pytest.raises(E, match="^samples are complex: pass iq=True$"):
        rx.decode_stream(np.zeros(500, np.complex64), 44100, resample=True)
    with pytest.raises(E, match="dtype complex64 is not taken at a wide rate"):
        rx.decode_stream(np.zeros(500, np.complex64), 240000)
    with pytest.raises(E, match="^samples: 2 streams at 240000 Hz -- a wide rate takes one stream$"):
        rx.decode_stream(np.zeros((2, 500, 2), np.int16), 240000, iq=True)
    with pytest.raises(E, match="^samples: 2 streams at 44100 Hz -- a resampled rate takes one stream$"):
        rx.decode_stream(np.zeros((2, 500), np.int16), 44100, resample=True)
    with pytest.raises(E, match=r"^src: \[0, 1\] -- a wide rate takes one stream, every channel reads stream 0$"):
        rx.decode_stream(np.zeros((500, 2), np.int8), 240000, iq=True, dial_offsets_hz=(0.0, 1.0), src=[0, 1])
    with pytest.raises(E, match=r"^src: \[1\] -- a resampled rate takes one stream"):
        rx.decode_stream(np.zeros(500, np.int16), 44100, src=[1], resample=True)
    with pytest.raises(E, match="rate 1000 is taken by none of"):
        rx.decode_stream(np.zeros(500, np.int16), 1000, resample=True)
    with pytest.raises(E, match="^dial_offsets_hz: at least one channel$"):
        rx.decode_stream(np.zeros(500, np.int16), 48000, dial_offsets_hz=())
    with pytest.raises(E, match=r"^src: 3 streams and 2 channels -- say which stream each channel reads$"):
        rx.decode_stream(np.zeros((3, 500), np.int16), 48000, dial_offsets_hz=(0.0, 1.0))
    with pytest.raises(E, match=r"^src: one stream index per channel \(2\), got 1$"):
        rx.decode_stream(np.zeros(500, np.int16), 48000, dial_offsets_hz=(0.0, 1.0), src=[0])
    with pytest.raises(E, match=r"^bands: one per channel \(2\), got 3$"):
        rx.decode_stream(np.zeros(500, np.int16), 48000, dial_offsets_hz=(0.0, 1.0), bands="abc")
    with pytest.raises(E, match=r"^recall: one list of earlier messages per channel \(2\), got 1$"):
        rx.decode_stream(np.zeros(500, np.int16), 48000, dial_offsets_hz=(0.0, 1.0), recall=[[]])
    with pytest.raises(TypeError, match=r"^decode_stream\(\) got an unexpected keyword argument 'n_threads'$"):
        rx.decode_stream(np.zeros(500, np.int16), 48000, n_threads=2)
    assert tape.take() == [] and tape.take_pkg() == []


# ---- poll, 12 kHz
def live_frame(rx, name, t_now, early=0):
    rx.audio_in._ready.append((load_golden(name)[0], t_now, early))


LIVE_PKG = ("package_batch", {"n_threads": 1, "table": "table", "rows": "plain"})
LIVE_PKG_RECALL = ("package_batch_recall", {"n_threads": 1, "table": "table", "rows": "plain"})


def test_poll_early_and_complete_pass(tape):
    cb = []
    rx = rx_of(cb, max_frames=1)
    rx.set_band("20m")
    tape.push(NAMES[:1], NAMES[:1])
    live_frame(rx, "test_08", 15013.6, 340)
    early = rx.poll()
    assert tape.take() == ["decode_batch(1)"] and tape.take_pkg() == [LIVE_PKG] and tape.tables == [rx.call_hashes]
    assert len(early) == 14 and all(d["early"] is True and d["cyclestart_string"] == "700101_041000" for d in early)
    live_frame(rx, "test_08", 15015.0)
    rest = rx.poll()
    assert tape.take() == ["decode_batch(1)"] and tape.take_pkg() == [LIVE_PKG]
    assert len(rest) == 7 and all(d["early"] is False and d["cyclestart_string"] == "700101_041000" for d in rest)
    assert sorted(got(early) + got(rest)) == sorted(texts("test_08")) and [t for t in texts("test_08") if t in got(rest)] == got(rest)
    assert all("OSD" not in d["decode_notes"] for d in early)
    assert all(d["band"] == "20m" and d["their_tx_cycle"] == 0 and "channel" not in d and "recall" not in d for d in early + rest)
    assert len(cb) == 21 and all(a is b for a, b in zip(cb, early + rest))
    assert len(tape.handles) == 2 and [h.max_frames for h in tape.handles] == [1, 1]          # the main handle and the live one
    # two frames waiting: both are decoded by one poll, in order; the next cycle has the other parity
    tape.push(NAMES[1:], NAMES[:1])
    live_frame(rx, "test_09", 15030.1)
    live_frame(rx, "test_08", 15045.2)
    out = rx.poll()
    # ... and one call-hash table for the stream: test_09 brings the call that test_08's hashed message lacked in the first cycle
    assert "<...> DL8RCH JN68" in texts("test_08") and "<OR18OSB> DL8RCH JN68" in got(out)
    assert [t.replace("<OR18OSB>", "<...>") for t in got(out)] == texts("test_09") + texts("test_08")
    assert tape.take() == ["decode_batch(1)"] * 2
    assert [d["their_tx_cycle"] for d in out] == [1] * 20 + [0] * 21
    assert rx.poll() == [] and tape.take() == []


def test_poll_recall_reports_blanker(tape):
    rx = rx_of(max_frames=1, recall=True, reports=True, noise_blanker=3.0)
    staged = ["blank_host(1)", "staging_ptr", "enqueue(1)", "fetch(1)"]
    tape.push(*[NAMES[:1]] * 6)
    live_frame(rx, "test_08", 15015.0)
    out = rx.poll()
    assert tape.take() == staged + ["fetch_reports(1)"] and tape.take_pkg() == [LIVE_PKG]          # no history yet: no recall
    assert len(out) == 21 and all(d["recall"] is False and d["report"] is None and d["early"] is False for d in out)
    assert tape.blank_params == (768, 6, 6) and rx.blanker_stats.shape == (1, 4)
    live_frame(rx, "test_08", 15043.6, 340)                       # an early pass: no recall, though the cycle 30 s back has history
    assert len(rx.poll()) == 14
    assert tape.take() == staged + ["fetch_reports(1)"] and tape.take_pkg() == [LIVE_PKG]
    live_frame(rx, "test_08", 15045.0)
    out = rx.poll()
    assert tape.take() == ["set_recall([19])"] + staged + ["fetch_recall(1)", "fetch_reports(1)"] and tape.take_pkg() == [LIVE_PKG_RECALL]
    assert len(out) == 7 and set(tape.tables) == {rx.call_hashes}
    assert sorted(rx._recall_hist) == [15000, 15030] and sorted(rx._cycle_seen) == [15000, 15030]
    # history and duplicate filters are pruned: the recall history keeps 30 s, the filter 60 s
    live_frame(rx, "test_08", 15060.0)                            # the cycle that starts at 15045: its partner 30 s back was not decoded
    assert len(rx.poll()) == 21 and tape.take() == staged + ["fetch_reports(1)"]
    assert sorted(rx._recall_hist) == [15030, 15045] and sorted(rx._cycle_seen) == [15000, 15030, 15045]
    live_frame(rx, "test_08", 15105.0)
    assert len(rx.poll()) == 21 and tape.take() == staged + ["fetch_reports(1)"]
    assert sorted(rx._recall_hist) == [15090] and sorted(rx._cycle_seen) == [15030, 15045, 15090]
    live_frame(rx, "test_08", 15135.0)
    assert len(rx.poll()) == 21 and tape.take()[0] == "set_recall([19])"
    assert sorted(rx._recall_hist) == [15090, 15120] and sorted(rx._cycle_seen) == [15090, 15120]


def test_poll_message_types(tape):
    rx = rx_of(max_frames=1, msg_types="all")
    tape.push(NAMES[:1])
    live_frame(rx, "test_08", 15015.0)
    assert got(rx.poll()) == texts("test_08")
    assert tape.take_pkg() == [("package_batch_ext", {"n_threads": 1, "table": "table", "mask": _lib.MT_ALL, "rows": "ext"})]


# ---- poll, wide input
def wide_rx(cb=None, **kw):
    return rx_of(cb, max_frames=1, sample_rate=48000, iq=True, dial_offsets_hz=(-1000, 2000), bands=("a", "b"), **kw)


def test_poll_wide(tape):
    cb = []
    rx = wide_rx(cb, recall=True, noise_blanker=True)
    w = rx.wide_in
    assert (w.n_channels, w.wide, w.rat, w.bands, w.dials, w.iq) == (2, False, False, ["a", "b"], [-1000.0, 2000.0], True)
    staged = ["blank(2)"] + STAGED
    tape.push(*[NAMES] * 6)
    w._ready.append((1000, 340, 0, 163200))
    early = rx.poll()
    assert tape.take() == ["ddc_stream_frame(0,163200)"] + staged and tape.take_pkg() == [LIVE_PKG] and tape.tables == [rx.call_hashes]
    assert [d["channel"] for d in early] == [0] * 14 + [1] * 18 and all(d["early"] is True for d in early)
    assert tape.handles[-1].max_frames == 2 and len(tape.handles) == 2
    w._ready.append((1000, 0, 0, 180000))
    rest = rx.poll()
    assert tape.take() == ["ddc_stream_frame(0,180000)"] + staged and tape.take_pkg() == [LIVE_PKG]
    # (channel 0 delivers its hashed message twice: by the complete pass channel 1 has brought the call into the shared table)
    assert [d["channel"] for d in rest] == [0] * 8 + [1] * 2 and all(d["early"] is False for d in rest)
    assert got(early).count("<...> DL8RCH JN68") == 1 and got(rest).count("<OR18OSB> DL8RCH JN68") == 1
    for j, nm in enumerate(NAMES):
        ch = [d for d in early + rest if d["channel"] == j]
        assert {t.replace("<OR18OSB>", "<...>") for t in got(ch)} == set(texts(nm)) and {d["band"] for d in ch} == {"ab"[j]}
        assert all(d["cyclestart_string"] == "700101_041000" and d["their_tx_cycle"] == 0 and d["recall"] is False for d in ch)
    assert len(cb) == 42 and all(a is b for a, b in zip(cb, early + rest))
    assert tape.blank_params == (2048, 6, 6) and rx.blanker_stats.shape == (2, 4)
    # 30 s later: recall in front and behind; an early pass of that cycle has none
    w._ready += [(1002, 340, 360000, 163200), (1002, 0, 360000, 180000)]
    out = rx.poll()
    assert tape.take() == ["ddc_stream_frame(360000,163200)"] + staged + \
        ["set_recall([19, 19])", "ddc_stream_frame(360000,180000)"] + staged + ["fetch_recall(2)"]
    assert tape.take_pkg() == [LIVE_PKG, LIVE_PKG_RECALL] and len(out) == 41
    assert [sorted(s) for s in w.seen] == [[15000, 15030]] * 2 and [sorted(s) for s in w.recall_hist] == [[15000, 15030]] * 2
    assert rx._cycle_seen == {} and rx._recall_hist == {}
    # recall is asked for when at least one channel has history, and not otherwise
    del w.recall_hist[1][15030]
    w._ready.append((1004, 0, 720000, 180000))
    assert len(rx.poll()) == 41
    assert tape.take() == ["set_recall([19, 0])", "ddc_stream_frame(720000,180000)"] + staged + ["fetch_recall(2)"]
    w._ready.append((1007, 0, 1260000, 180000))
    out = rx.poll()
    assert tape.take() == ["ddc_stream_frame(1260000,180000)"] + staged and tape.take_pkg()[-1] == LIVE_PKG
    assert all(d["their_tx_cycle"] == 1 and d["cyclestart_string"] == "700101_041145" for d in out)
    assert [sorted(s) for s in w.recall_hist] == [[15105]] * 2 and [sorted(s) for s in w.seen] == [[15060, 15105]] * 2


def test_poll_wide_plain(tape):
    """No opt-ins, no bands: the receiver's own band, and the 12 kHz queue is served in front of the wide one."""
    rx = rx_of(max_frames=1, sample_rate=96000, dial_offsets_hz=(0.0,), reports=True)
    rx.set_band("40m")
    tape.push(NAMES[:1], NAMES[1:])
    rx.wide_in._ready.append((1000, 0, -3000, 180000))
    live_frame(rx, "test_08", 15015.0)
    out = rx.poll()
    assert tape.take() == ["decode_batch(1)", "fetch_reports(1)", "ddc_stream_frame(-3000,180000)", "staging_ptr", "enqueue(1)", "fetch(1)",
                           "fetch_reports(1)"]
    assert got(out) == texts("test_08") + texts("test_09") and ["channel" in d for d in out] == [False] * 21 + [True] * 20
    assert all(d["band"] == "40m" and d["report"] is None and "recall" not in d for d in out)


def test_start_builds_the_wide_input_like_the_constructor(tape):
    rx = rx_of(max_frames=1)
    assert rx.wide_in is None
    rx.start(sample_rate=240000, iq=True, dial_offsets_hz=(1.0, 2.0), bands=("x", "y"), t_first=15000.0)
    try:
        w = rx.wide_in
        assert (w.sample_rate, w.iq, w.dials, w.bands, w.t_first, w.wide, w.rat, w.n_channels) == \
            (240000, True, [1.0, 2.0], ["x", "y"], 15000.0, True, False, 2)
    finally:
        rx.stop()
    rx = rx_of(max_frames=1, sample_rate=44100, resample=True, t_first=3.0)
    assert (rx.wide_in.rat, rx.wide_in.wide, rx.wide_in.t_first, rx.wide_in.bands) == (True, False, 3.0, None)


# ---- the live wide input on its three front ends: how the stream is opened, how chunks and the zeros of flush() reach it
@pytest.mark.parametrize("rate, kw, chunk, opened, pushes", [
    (48000, dict(iq=True, dial_offsets_hz=(1.0, 2.0)), np.ones((2, 50000, 2), np.int16),
     f"ddc_stream_open({ddc.IQ_I16},48000,2,[0, 1],[1.0, 2.0])",
     ["ddc_stream_push((2, 48000, 2),int16,1)", "ddc_stream_push((2, 2000, 2),int16,1)"] + ["ddc_stream_push((2, 4032, 2),int16,0)"] * 2),
    (24000, dict(dial_offsets_hz=(1.0, 2.0)), np.ones(3000, np.float64),
     f"ddc_stream_open({ddc.REAL_F32},24000,1,[0, 0],[1.0, 2.0])",
     ["ddc_stream_push((1, 3000),float32,1.0)"] + ["ddc_stream_push((1, 2016),float32,0.0)"] * 2),
    (240000, dict(iq=True, dial_offsets_hz=(1.0, 2.0)), np.ones((1, 30000, 2), np.uint8),
     f"ddc_wide_stream_open({ddc_wide.IQ_U8},240000,[1.0, 2.0])",
     ["ddc_wide_stream_push((30000, 2),uint8,1)"] + ["ddc_wide_stream_push((20160, 2),uint8,128)"] * 2),
    (240000, dict(dial_offsets_hz=(7.0,)), np.ones(30000, np.int16),
     f"ddc_wide_stream_open({ddc_wide.REAL_I16},240000,[7.0])",
     ["ddc_wide_stream_push((30000,),int16,1)"] + ["ddc_wide_stream_push((20160,),int16,0)"] * 2),
    (44100, dict(dial_offsets_hz=(7.0,), resample=True), np.ones(5000, np.float32),
     f"ddc_rat_stream_open({ddc_rat.REAL_F32},44100,[7.0])",
     ["ddc_rat_stream_push((5000,),float32,1.0)"] + ["ddc_rat_stream_push((3705,),float32,0.0)"] * 2),
    (2048000, dict(iq=True, dial_offsets_hz=(7.0,), resample=True), np.ones((300000, 2), np.uint8),
     f"ddc_rat_stream_open({ddc_rat.IQ_U8},2048000,[7.0])",
     ["ddc_rat_stream_push((300000, 2),uint8,1)"] + ["ddc_rat_stream_push((172032, 2),uint8,128)"] * 2),
    (2048000, dict(iq=True, dial_offsets_hz=(7.0,), resample=True), np.ones(300000, np.complex64),
     f"ddc_rat_stream_open({ddc_rat.IQ_F32},2048000,[7.0])",
     ["ddc_rat_stream_push((300000, 2),float32,1.0)"] + ["ddc_rat_stream_push((172032, 2),float32,0.0)"] * 2)])
def test_wide_in_front_ends(tape, rate, kw, chunk, opened, pushes):
    rx = rx_of(max_frames=1, sample_rate=rate, t_first=15000.0, **kw)
    w = rx.wide_in
    w.push(chunk)
    w.flush()
    assert tape.take() == [opened] + pushes
    assert w.n_pushed == (chunk.shape[1] if chunk.ndim == 3 else chunk.shape[0]) and w.m_produced >= w._outputs(w.n_pushed)
    assert tape.handles[-1].max_frames == w.n_channels


def test_wide_in_refusals(tape):
    E = _lib.Ft8rxError
    with pytest.raises(E, match="^samples are complex: pass iq=True$"):
        rx_of(sample_rate=48000).wide_in.push(np.zeros(100, np.complex64))
    with pytest.raises(E, match="^samples are complex: pass iq=True$"):
        rx_of(sample_rate=44100, resample=True).wide_in.push(np.zeros(100, np.complex64))
    with pytest.raises(E, match="a wide rate takes one stream, every channel reads stream 0$"):
        receiver._wide_in.WideIn(rx_of(), 240000, iq=True, src=[1]).push(np.zeros((100, 2), np.int16))
    with pytest.raises(E, match="^samples: 2 streams at 240000 Hz -- a wide rate takes one stream$"):
        rx_of(sample_rate=240000, iq=True).wide_in.push(np.zeros((2, 100, 2), np.int16))
    with pytest.raises(E, match="^src: 3 streams and 2 channels"):
        rx_of(sample_rate=48000, dial_offsets_hz=(0.0, 1.0)).wide_in.push(np.zeros((3, 100), np.int16))
    assert tape.take() == []
    w = rx_of(sample_rate=48000).wide_in
    w.push(np.zeros((1, 100), np.int16))
    with pytest.raises(E, match="^push: 2 streams, the source began with 1$"):
        w.push(np.zeros((2, 100), np.int16))
