"""The down-converter on the GPU (ft8rx_ddc) against its float64 twin (pyft8_amd/ddc.py: reference), its
invariances, the decode of down-converted channels through Receiver.decode_stream, and its refusals.

RMS error of the float32 output against the twin, full-scale random input (counts; measured on an MI355X):
printed by test_twin for every kind and rate."""

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

import ddc_cases as cases
from conftest import load_golden
from pyft8_amd import _lib, ddc
from pyft8_amd.receiver import Receiver

pytestmark = pytest.mark.gpu

NSAMP = 180000
SRC = [1, 0, 1]
KINDS_RATES = [(k, 12000 * D) for k in range(4) for D in (1, 2, 4, 8, 16) if not (k == ddc.REAL_I16 and D == 1)]
F32_SCALE = 0.375                    # float kinds carry the int16 values times 3/8: exact in float32, so one twin serves both


def dials(rate):
    """negative and within 1 kHz of -rate/2; positive; within 1 kHz of +rate/2 (fc = dial + 3000 wraps)"""
    return [-0.5 * rate + 400.5, 0.11 * rate + 33.3, 0.5 * rate - 700.25]


_data, _twin = {}, {}


def streams(D):
    """Two streams of full-scale random IQ int16, n neither the full length nor a multiple of D: [2, n, 2]"""
    if D not in _data:
        n = NSAMP * D - 1237
        assert n % D != 0 or D == 1
        rng = np.random.Generator(np.random.Philox(key=0xDDC0 + D))
        x = rng.integers(-32768, 32768, size=(2, n, 2), dtype=np.int64).astype(np.int16)
        x[0, :3], x[1, -3:] = [[32767, -32768]] * 3, [[-32768, -32768]] * 3          # the corners of the range, at both ends
        x.setflags(write=False)
        _data[D] = x
    return _data[D]


def samples(kind, D):
    x = streams(D)
    if kind == ddc.IQ_I16:
        return x
    if kind == ddc.REAL_I16:
        return np.ascontiguousarray(x[:, :, 0])
    f = x.astype(np.float32) * np.float32(F32_SCALE)
    return f if kind == ddc.IQ_F32 else np.ascontiguousarray(f[:, :, 0])


def twin(iq, D):
    """The twin's three outputs for the int16 data (IQ, or its I component as a real stream): y [3, 180000], f_mixed [3]"""
    key = (bool(iq), D)
    if key not in _twin:
        x, rate = streams(D), 12000 * D
        kind = ddc.IQ_I16 if iq else ddc.REAL_F32            # (the twin reads real int16 and real float32 alike)
        res = [ddc.reference(x[s] if iq else x[s, :, 0], kind, rate, f) for s, f in zip(SRC, dials(rate))]
        y = np.stack([r[0] for r in res])
        y.setflags(write=False)
        _twin[key] = (y, np.array([r[1] for r in res]))
    return _twin[key]


def bound(kind, rate, gain, xmax):
    """(n_macs + 16) 2^-23 G max|x|: n_macs = the multiply-adds on the path into one output (len(h1) + len(h2): each of the two sums
    may be taken in any order), G = gain g sum|h1| sum|h2|.  Each float32 operation adds at most 2^-24 of the magnitudes summed so
    far; the 16 covers the two rounded phasor tables, their product, the mixing product and the final scaling."""
    h1, h2 = ddc.taps(rate, 1), ddc.taps(rate, 2)
    g = 1.0 if ddc.is_iq(kind) else 2.0
    G = gain * g * (np.abs(h1.astype(np.float64)).sum() if len(h1) else 1.0) * np.abs(h2.astype(np.float64)).sum()
    return (len(h1) + len(h2) + 16) * 2.0 ** -23 * G * xmax


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle(device=0, max_frames=3)
    yield h
    h.close()


@pytest.mark.parametrize("kind,rate", KINDS_RATES, ids=[f"{ddc.KIND_NAMES[k].replace(' ', '_')}-{r}" for k, r in KINDS_RATES])
def test_twin(handle, kind, rate):
    D = rate // 12000
    x = samples(kind, D)
    y_ref, f_ref = twin(ddc.is_iq(kind), D)
    scale = F32_SCALE if kind in (ddc.REAL_F32, ddc.IQ_F32) else 1.0
    fm, y = handle.ddc(x, kind, rate, SRC, dials(rate), want_float=True)
    a = handle.download_audio(handle.staging_ptr(), 3)
    xc = x.astype(np.float64)
    xmax = float(np.sqrt((xc ** 2).sum(axis=2)).max() if ddc.is_iq(kind) else np.abs(xc).max())
    err = y.astype(np.float64) - scale * y_ref
    lim = bound(kind, rate, 1.0, xmax)
    print(f"ddc twin {ddc.KIND_NAMES[kind]} {rate} Hz: max |err| {np.abs(err).max():.5f}, rms {np.sqrt((err ** 2).mean()):.6f} counts, "
          f"bound {lim:.4f}, rms of y {y.std():.1f}")
    assert np.array_equal(fm, f_ref)
    assert y.shape == (3, NSAMP) and np.isfinite(y).all() and y.std() > 1000 * scale          # a real signal came out
    assert np.abs(err).max() <= lim
    assert np.array_equal(a, cases.to_frame(y))                                      # the frame is rint + saturation of the GPU's own y
    tail = (x.shape[1] + D - 1) // D + 200                                           # beyond the input and the filters: the zero tail
    assert not y[:, tail:].any() and not a[:, tail:].any()


def test_saturation(handle):
    """gain drives the output past full scale: -32768 / 32767, never a wrap"""
    rate, gain = 48000, 24.0
    x = samples(ddc.IQ_I16, 4)
    y_ref, _ = twin(True, 4)
    fm, y = handle.ddc(x, ddc.IQ_I16, rate, SRC, dials(rate), gain=gain, want_float=True)
    a = handle.download_audio(handle.staging_ptr(), 3)
    assert y.max() > 2 * 32767 and y.min() < -2 * 32768
    assert np.array_equal(a, cases.to_frame(y))
    assert (a == 32767).sum() > 1000 and (a == -32768).sum() > 1000
    xmax = float(np.sqrt((x.astype(np.float64) ** 2).sum(axis=2)).max())
    assert np.abs(y - gain * y_ref).max() <= bound(ddc.IQ_I16, rate, gain, xmax)


def test_invariance(handle):
    rate = 96000
    x, f = samples(ddc.IQ_I16, 8), dials(rate)
    fm3, y3 = handle.ddc(x, ddc.IQ_I16, rate, SRC, f, want_float=True)
    a3 = handle.download_audio(handle.staging_ptr(), 3)
    assert np.array_equal(fm3, twin(True, 8)[1])
    # two runs agree
    fm3b, y3b = handle.ddc(x, ddc.IQ_I16, rate, SRC, f, want_float=True)
    assert y3b.tobytes() == y3.tobytes() and np.array_equal(fm3, fm3b)
    assert handle.download_audio(handle.staging_ptr(), 3).tobytes() == a3.tobytes()
    # the host entry agrees with the device entry
    fmh = handle.ddc(x, ddc.IQ_I16, rate, SRC, f)
    assert np.array_equal(fmh, fm3) and handle.download_audio(handle.staging_ptr(), 3).tobytes() == a3.tobytes()
    # an output computed alone (from its stream alone, too) is the same bytes
    for j in range(3):
        fm1, y1 = handle.ddc(x[SRC[j]:SRC[j] + 1], ddc.IQ_I16, rate, [0], [f[j]], want_float=True)
        assert y1[0].tobytes() == y3[j].tobytes() and fm1[0] == fm3[j]
        assert handle.download_audio(handle.staging_ptr(), 1)[0].tobytes() == a3[j].tobytes()


@pytest.fixture(scope="module")
def rx():
    r = Receiver("", None, max_frames=2)
    yield r
    r.close()


@pytest.mark.parametrize("i,D", [(0, 4), (1, 4), (2, 4), (0, 16), (0, 1)])
def test_decode_stream(rx, i, D):
    """Two FT8 channels in one IQ stream (with a strong tone just outside each): every channel decodes to the message set of its
    original 12 kHz frame; at D = 1 channel a alone."""
    iq, offs, originals = cases.recipe(i, D, only_a=(D == 1))
    bands = ["20m", "17m"][:len(offs)]
    want = rx.decode_frames(np.stack(originals))
    got = rx.decode_stream(iq[None], 12000 * D, iq=True, dial_offsets_hz=offs, bands=bands)
    assert len(got) == len(offs)
    for j in range(len(offs)):
        texts, ref = {" ".join(d["msg_tuple"]) for d in got[j]}, {" ".join(d["msg_tuple"]) for d in want[j]}
        print(f"ddc decode i={i} D={D} channel {j}: {len(texts)} messages, original frame {len(ref)}")
        assert texts == ref and len(ref) >= 5
        assert all(d["band"] == bands[j] for d in got[j])
        assert all(0.0 < d["fHz"] < 3000.0 for d in got[j])                           # the audio frequency inside the channel


def test_decode_stream_passes(rx):
    """passes=2 works on the frames ft8rx_ddc left in the staging buffer: they are ordinary frames (the same call on a host copy of
    them gives the same messages)"""
    iq, offs, _ = cases.recipe(0, 4)
    one = rx.decode_stream(iq[None], 48000, iq=True, dial_offsets_hz=offs)
    h = rx._handle(2)
    h.ddc(iq[None], ddc.IQ_I16, 48000, [0, 0], offs)
    frames = h.download_audio(h.staging_ptr(), 2)
    two = rx.decode_stream(iq[None], 48000, iq=True, dial_offsets_hz=offs, passes=2)
    want = rx.decode_frames(frames, passes=2)
    for j in range(2):
        t1, t2 = [" ".join(d["msg_tuple"]) for d in one[j]], [" ".join(d["msg_tuple"]) for d in two[j]]
        assert t2[:len(t1)] == t1                                                     # the first pass, then what subtraction adds
        assert t2 == [" ".join(d["msg_tuple"]) for d in want[j]]
        assert [d["decode_notes"] for d in two[j]] == [d["decode_notes"] for d in want[j]]


def test_refusals_and_untouched_default_path(handle):
    audio = np.stack([load_golden(n)[0] for n in ("test_08", "synth_000000")])
    before = handle.decode_batch(audio)
    L, h = handle._L, handle._h
    x = np.zeros((2, 1000, 2), np.int16)
    src, f, fm = np.zeros(4, np.int32), np.zeros(4, np.float64), np.zeros(4, np.float64)

    def call(kind=ddc.IQ_I16, rate=48000, n_streams=2, stride=1000, n=1000, n_out=1, src=src):
        rc = L.ft8rx_ddc_host(h, x.ctypes.data, kind, rate, n_streams, stride, n, n_out, src.ctypes.data, f.ctypes.data, 1.0, fm.ctypes.data)
        return rc, L.ft8rx_last_error(h).decode()

    assert call()[0] == 0
    for kw, word in (({"kind": 4}, "kind"), ({"kind": -1}, "kind"), ({"rate": 44100}, "rate_hz"), ({"rate": 384000}, "rate_hz"),
                     ({"kind": ddc.REAL_I16, "rate": 12000}, "real int16"), ({"n_out": 4}, "n_out"), ({"n_out": 0}, "n_out"),
                     ({"src": np.array([2, 0, 0, 0], np.int32)}, "src[0]"), ({"src": np.array([-1, 0, 0, 0], np.int32)}, "src[0]"),
                     ({"n": 180000 * 4 + 1, "stride": 180000 * 4 + 1}, "n_samples"), ({"n": 1001}, "stream_stride")):
        rc, text = call(**kw)
        assert rc == -1 and word in text, (kw, rc, text)
    f[0] = 24000.0
    rc, text = call()
    assert rc == -1 and "f_dial_hz[0]" in text
    f[0] = 0.0
    rc = L.ft8rx_ddc(h, None, ddc.IQ_I16, 48000, 2, 1000, 1000, 1, src.ctypes.data, f.ctypes.data, 1.0, None, None, None)
    assert rc == -1 and "d_in" in L.ft8rx_last_error(h).decode()
    with pytest.raises(_lib.Ft8rxError, match="kind"):
        handle.ddc(x, 7, 48000, [0], [0.0])
    assert call()[0] == 0                                                             # and a good call still runs
    after = handle.decode_batch(audio)
    # (rows beyond a frame's counts are whatever the result slot held, and the event log is written in arrival order: compare the
    # records the counts cover and the events as a set)
    assert before[1].tobytes() == after[1].tobytes() and before[3].tobytes() == after[3].tobytes() and before[1].min() > 0
    for fr in range(2):
        nc, ne = int(before[1][fr]), min(int(before[3][fr]), _lib.EVENT_CAP)
        assert before[0][fr, :nc].tobytes() == after[0][fr, :nc].tobytes()
        assert sorted(e.tobytes() for e in before[2][fr, :ne]) == sorted(e.tobytes() for e in after[2][fr, :ne])
