"""Float32 frames without a GPU: what the Python surface refuses and how it prepares float frames, the new
symbols of the prototype table against the header, and the float64 twin's word on the quiet wide stream of the GPU tests."""
import os

import numpy as np
import pytest

import float_frames_cases as F
from conftest import ROOT
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
