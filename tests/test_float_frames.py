"""Float32 frames without a GPU: what the Python surface refuses and how it prepares float frames, the new
symbols of the prototype table against the header, the float64 twin's word on the quiet wide stream of the GPU tests -- and the
oracle's float entries (ft8o_spectrogram_f32, ft8o_cycle_spectrum_f32, ft8o_decode_frame_f32): equal to the int16 entries on
integer-valued floats, held to float64 numpy on the level and edge frames of the GPU tests, and the conditions those frames meet."""
import os

import numpy as np
import pytest

import float_frames_cases as F
import oracle as O
from conftest import ROOT, load_golden
from pyft8_amd import _abi, _lib, blanker, ddc, ddc_wide, receiver as R
from test_abi import c_prototypes, mismatches

NSAMP = 180000
F32_ENTRIES = ("ft8rx_enqueue_batch_f32", "ft8rx_enqueue_batch_host_f32", "ft8rx_decode_batch_f32", "ft8rx_decode_messages_f32",
               "ft8rx_staging_audio_f32", "ft8rx_spectrogram_f32", "ft8rx_cycle_spectrum_f32", "ft8rx_ddc_stream_frame_f32", "ft8rx_subtract_f32")


def test_float_arrays_without_the_flag_are_refused_as_before():
    with pytest.raises(_lib.Ft8rxError, match=r"frame 0: samples must be integers in int16 range \(got float64\)"):
        R.frames_from_ragged([np.array([1.5])])
    with pytest.raises(_lib.Ft8rxError, match=r"frame 0: samples must be integers in int16 range \(got float32\)"):
        R._as_frames(np.zeros((2, NSAMP), np.float32))
    assert R.frames_from_ragged([np.array([3, -4])]).dtype == np.int16                # ... and integers are taken as before


def test_frames_from_ragged_f32_pads_and_rounds_once():
    a = np.array([0.1, 1.0 + 2.0 ** -30, -2.0 ** -140, 3.0e-39], np.float64)
    b = np.arange(5, dtype=np.float32) * np.float32(0.25)
    out = R.frames_from_ragged_f32([a, b, np.zeros(0, np.float32)])
    assert out.dtype == np.float32 and out.shape == (3, NSAMP) and out.flags["C_CONTIGUOUS"]
    assert out[0, :4].tobytes() == a.astype(np.float32).tobytes() and out[0, 1] == 1.0 and out[0, 0] == np.float32(0.1)      # one rounding
    assert out[1, :5].tobytes() == b.tobytes()                                          # float32 as it is
    assert not out[0, 4:].any() and not out[1, 5:].any() and not out[2].any()           # zeros behind a short frame
    one = R.frames_from_ragged_f32(np.full(NSAMP, 0.5))                                 # one frame as a vector
    assert one.shape == (1, NSAMP) and (one == 0.5).all()
    two = R._as_frames_f32(np.ones((2, 7)))                                             # [B, n]
    assert two.shape == (2, NSAMP) and two[:, :7].all() and not two[:, 7:].any()


def test_frames_from_ragged_f32_refusals():
    ok = np.zeros(10, np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(_lib.Ft8rxError, match="frame 1: non-finite"):
            R.frames_from_ragged_f32([ok, np.array([0.0, bad, 1.0], np.float32)])
    with pytest.raises(_lib.Ft8rxError, match="frame 0: non-finite"):                   # a float64 beyond the float32 range
        R.frames_from_ragged_f32([np.array([1e39])])
    with pytest.raises(_lib.Ft8rxError, match=f"frame 1: {NSAMP + 1} samples > {NSAMP}"):
        R.frames_from_ragged_f32([ok, np.zeros(NSAMP + 1, np.float32)])
    with pytest.raises(_lib.Ft8rxError, match=r"frame 0: float_frames=True takes float32 or float64 samples \(got int16\)"):
        R.frames_from_ragged_f32([np.zeros(4, np.int16)])
    with pytest.raises(_lib.Ft8rxError, match="frame 0: expected a 1-D array"):
        R.frames_from_ragged_f32([np.zeros((2, 2), np.float32)])
    with pytest.raises(_lib.Ft8rxError, match="float32"):
        _lib._audio_f32(np.zeros((1, NSAMP), np.int16), "audio must be float32, got {shape}")
    with pytest.raises(_lib.Ft8rxError, match=r"\(1, 5\)"):
        _lib._audio_f32(np.zeros((1, 5), np.float32), "audio must be float32, got {shape}")
    assert _lib._audio_f32(np.full(NSAMP, 0.1), "{shape}").dtype == np.float32


def test_noise_blanker_is_refused_with_float_frames_naming_both():
    R.refuse_float_with_blanker(False, blanker.params(True))
    R.refuse_float_with_blanker(True, blanker.params(None))
    with pytest.raises(_lib.Ft8rxError, match="float_frames=True is not supported together with noise_blanker"):
        R.refuse_float_with_blanker(True, blanker.params(True))


def test_keep_f32_values():
    assert [_lib._keep_f32(v) for v in (False, 0, None, True, 1, 2)] == [0, 0, 0, 1, 1, 2]


def test_new_symbols_match_the_header():
    text = open(os.path.join(ROOT, "include", "ft8rx.h")).read()
    header = c_prototypes(text, r"ft8rx_\w+_f32")
    assert sorted(header) == sorted(F32_ENTRIES)
    assert mismatches({n: _abi.PROTOTYPES[n] for n in F32_ENTRIES}, header) == []
    twins = c_prototypes(text, r"ft8rx_\w+")
    for n in F32_ENTRIES:                                                               # each is its twin's prototype
        assert header[n] == twins[n[:-4]], n
    assert "FT8RX_DDC_KEEP_F32_FRAMES 2" in text


def test_built_library_exports_the_new_symbols():
    for wide in (False, True):
        L = _lib.lib(wide)
        for n in F32_ENTRIES:
            assert getattr(L, n).argtypes == list(_abi.PROTOTYPES[n][1]), n


def test_integer_frames_of_the_cases():
    a = F.int_frames()
    assert a.shape == (4, NSAMP) and a.dtype == np.int16 and not a[2].any()
    r = a[3].astype(np.int32)
    assert r.max() == 32767 and r.min() == -32768 and (r == -32767).any()
    assert a.astype(np.float32).astype(np.int16).tobytes() == a.tobytes()               # integer-valued floats


def test_quiet_streams_round_to_zero_frames_in_the_twin():
    """48 kHz: the quiet stream is the full one times 2^-20, and the twin's |y| stays far under half a count; 240 kHz: the twin's
    frames of the quiet wide stream are all zero, while the stream times 64 gives frames that are not"""
    q, full = F.quiet_stream(), F.full_stream()
    assert q.dtype == np.complex64 and (q.view(np.float32) * np.float32(2.0 ** 20)).tobytes() == full.view(np.float32).tobytes()
    for f in F.offsets():
        y, _ = ddc.reference(q, ddc.IQ_F32, F.RATE, f)
        assert 0.0 < np.abs(y).max() < 0.05
    x = F.wide_quiet_stream()
    assert x.dtype == np.int16 and np.abs(x).max() * F.WIDE_UP <= 32767
    kind = ddc_wide.kind_of(x, True)
    for f in F.wide_offsets():
        y, _ = ddc_wide.reference(x, kind, F.WIDE_RATE, f)
        print(f"wide channel at {f:.1f} Hz: max |y| {np.abs(y).max():.3f}, rms {y.std():.4f}")
        assert np.abs(y).max() < 0.5 and y.std() > 0.01
        assert not np.clip(np.rint(y), -32768, 32767).any()


# ---- the oracle's float entries
def _cand_key(c):
    return tuple(getattr(c, k) for k, _ in O.Cand._fields_)


def _texts(r):
    return [" ".join(m["msg_tuple"]) for m in r["msgs"]]


_decodes = {}


def _int_decode(name):
    if name not in _decodes:
        _decodes[name] = O.decode_frame(load_golden(name)[0])
    return _decodes[name]


def test_oracle_float_entries_equal_the_int16_entries_on_integer_valued_floats():
    """grid bytes, cycle spectrum bytes, candidate records (every field), events, messages -- on the four integer frames"""
    n_msgs = 0
    for a in F.int_frames():
        af = a.astype(np.float32)
        assert O.spectrogram_f32(af).tobytes() == O.spectrogram(a).tobytes()
        assert O.cycle_spectrum_f32(af).tobytes() == O.cycle_spectrum(a).tobytes()
        r, rf = O.decode_frame(a), O.decode_frame_f32(af)
        assert [_cand_key(c) for c in rf["cands"]] == [_cand_key(c) for c in r["cands"]]
        assert rf["n_events"] == r["n_events"] and [bytes(e) for e in rf["events"]] == [bytes(e) for e in r["events"]]
        assert rf["msgs"] == r["msgs"]
        n_msgs += len(r["msgs"])
    assert n_msgs >= 40
    aw = load_golden("test_08")[0]                                                      # the wide layouts
    wcfg = O.default_config(f0_hi=1280)
    assert O.spectrogram_f32(aw.astype(np.float32), wcfg).tobytes() == O.spectrogram(aw, wcfg).tobytes()
    assert O.spectrogram(aw, wcfg).shape == (O.GRID_ROWS, O.GRID_COLS_WIDE)


def _float64_grid(x):
    """window x rfft, 10 log10 max(|X|^2, 1e-24), rows 1 .. 375 (row r: the 3840 samples before sample 480 r, zeros before the start)"""
    xp = np.concatenate([np.zeros(3840), x.astype(np.float64)])
    w = np.hanning(3840).astype(np.float32).astype(np.float64)                          # the window is float32 in every statement
    seg = np.stack([xp[480 * r:480 * r + 3840] for r in range(1, 376)]) * w
    pw = np.abs(np.fft.rfft(seg, axis=1)[:, :O.GRID_COLS]) ** 2
    return 10.0 * np.log10(np.maximum(pw, 1e-24))


def _float64_spec(x):
    return np.fft.rfft(x.astype(np.float64), 192000)[:O.SPEC_BINS]


GRID_BOUND, SPEC_BOUND = 1e-3, 1e-5           # test_spectrogram_bit_exact, test_cycle_spectrum_bit_exact (tests/test_gpu_parity.py)


def _all_float_frames():
    return [(f"{n}@{lv}", x) for n, lv, x in F.level_frames()] + [(f"edge@{lv}", F.edge_frame(lv)) for lv in F.LEVELS]


def test_oracle_float_entries_against_float64_numpy():
    """Every level and edge frame: the grid within 1e-3 dB over the bins within 60 dB of their row's maximum, the cycle spectrum within
    1e-5 of its RMS -- the two bounds the int16 stages are held to against the reference's goldens.  Every grid value is finite and
    above -239.9 dB (none sits on the floor), so a loader that lost the quiet level or overflowed at the loud one would show."""
    frames = _all_float_frames()
    assert len(frames) == 9
    for label, x in frames:
        assert x.dtype == np.float32 and ((x.view(np.uint32) & 0xFF) != 0).mean() > 0.9, label    # more than 16 significant bits
        g = O.spectrogram_f32(x)[1:].astype(np.float64)
        assert np.isfinite(g).all() and g.min() > -239.9, (label, g.min(), g.max())
        ref = _float64_grid(x)
        strong = ref > ref.max(axis=1, keepdims=True) - 60.0
        e_grid = np.abs(g - ref)[strong].max()
        s = O.cycle_spectrum_f32(x).astype(np.complex128)
        sref = _float64_spec(x)
        e_spec = np.abs(s - sref).max() / np.sqrt(np.mean(np.abs(sref) ** 2))
        print(f"oracle against float64, {label}: grid {e_grid:.2e} dB over {strong.sum()} bins (min {g.min():.1f} dB, max {g.max():.1f} dB), "
              f"cycle spectrum {e_spec:.2e} of its rms")
        assert e_grid <= GRID_BOUND and e_spec <= SPEC_BOUND, (label, e_grid, e_spec)


def test_level_frames_decode_to_the_int16_messages():
    """The conditions the GPU chain test rests on, asserted on the oracle alone: every level frame gives the int16 frame's messages in
    the same order, at least 20 per frame"""
    for name, lv, x in F.level_frames():
        want = _texts(_int_decode(name))
        got = _texts(O.decode_frame_f32(x))
        print(f"{name}@{lv}: {len(got)} messages")
        assert got == want and len(got) >= 20, (name, lv)


def test_edge_frames_and_stage_batch():
    for lv, c in F.LEVELS.items():
        e, base = F.edge_frame(lv), F.level_frame(F.EDGE_BASE[lv], lv)
        big = np.float32(30000.0 * c)
        assert (e[:2] == big).all() and (e[-2:] == -big).all() and e[2:-2].tobytes() == base[2:-2].tobytes()
        assert np.log2(c) != np.rint(np.log2(c))                                        # no power of two
    b = F.stage_batch()
    assert b.shape == (4, NSAMP) and b.dtype == np.float32
    assert np.abs(b[0]).max() < 3e-5 and 1.5e9 < np.abs(b[1]).max() < 1.7e9 and 0.6 < np.abs(b[2]).max() < 0.71
    assert b[3].tobytes() == load_golden("test_08")[0].astype(np.float32).tobytes()


def test_reports_inputs_under_power_of_two_scaling():
    """The end-to-end reports test of tests/test_gpu_float_levels.py allows one message per frame to be left out because its record
    moved under the scaling by 2^-15 (the grid's log10f is not shifted exactly): the oracle says how many move on these inputs"""
    moved = []
    for a in F.int_frames():
        r, rf = O.decode_frame(a), O.decode_frame_f32(a.astype(np.float32) * np.float32(2.0 ** -15))
        assert _texts(rf) == _texts(r)
        key = lambda res, m: tuple(getattr(res["cands"][m["cand"]], k) for k in ("f0_idx", "h0_idx", "ttweak", "ftweak"))
        moved.append(sum(key(r, m) != key(rf, mf) for m, mf in zip(r["msgs"], rf["msgs"])))
    print(f"messages whose record moved under 2^-15, per frame: {moved}")
    assert max(moved) <= 1, moved
