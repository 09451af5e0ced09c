"""The handle calls of the wide live input and of decode_stream with panorama=, as literal traces without a GPU,
on the stand-in handle of tests/test_receiver_passes.py extended by the panorama's methods and the front ends' device pushes.  With the
keyword off the traces are that file's, untouched."""
import numpy as np
import pytest

import test_receiver_passes as trp
from pyft8_amd import _lib, ddc_wide, pan

PAN_BUF = 0x7A0000


@pytest.fixture
def tape(monkeypatch):
    t = trp.Tape()

    class Handle(trp.stand_in(t)):
        def pan_stream_open(self, kind, n_fft, n_avg, n_rows, n_origin=0, max_push=0):
            self.pan_cfg, self.pan_n = (kind, n_fft, n_avg), 0
            t.calls.append(f"pan_stream_open({kind},{n_fft},{n_avg},{n_rows},{n_origin},{max_push})")

        def pan_stream_push(self, samples=None, d_ptr=None, n=None):
            if d_ptr is None:
                n = len(samples)
                t.calls.append(f"pan_stream_push({samples.shape},{samples.dtype},{samples.reshape(-1)[0]})")
            else:
                t.calls.append(f"pan_stream_push(d_ptr={d_ptr:#x},n={n})")
            self.pan_n += n
            return PAN_BUF, pan.rows_done(0, self.pan_n, self.pan_cfg[1], self.pan_cfg[2])[1]

        def pan_stream_read(self, r_first, n):
            t.calls.append(f"pan_stream_read({r_first},{n})")
            return np.full((n, pan.bins(self.pan_cfg[0], self.pan_cfg[1])), 2.0, np.float32), np.full((n, 2), 3, np.int64)

        def pan(self, samples, kind, n_fft, n_avg, d_ptr=None, n=None):
            t.calls.append(f"pan({None if samples is None else samples.shape},{kind},{n_fft},{n_avg},d_ptr={d_ptr},n={n})")
            n = len(samples) if samples is not None else n
            return np.ones((n // n_fft // n_avg, pan.bins(kind, n_fft)), np.float32), None

        def ddc_wide_stream_push(self, a, d_ptr=None, n=None):
            if d_ptr is None:
                return super().ddc_wide_stream_push(a)
            t.calls.append(f"ddc_wide_stream_push(d_ptr={d_ptr:#x},n={n})")
            self.n_in += n
            return max(0, self.n_in * 12000 // self.rate - 1200) // 1008 * 1008

    monkeypatch.setattr(_lib, "Handle", Handle)
    return t


def test_wide_in_with_panorama_feeds_the_front_end_from_the_panorama_buffer(tape):
    """every real chunk: one host push into the panorama stream, the front end's device push on the address it returned, one read of
    the rows that push finished; the zeros of flush() are no source samples and go to the front end alone"""
    rx = trp.rx_of(max_frames=1, sample_rate=240000, t_first=15000.0, iq=True, dial_offsets_hz=(1.0, 2.0), panorama={"n_fft": 256, "n_avg": 50, "rows": 3})
    w = rx.wide_in
    assert w.panorama is None and rx.panorama is None
    w.push(np.ones((1, 30000, 2), np.uint8))
    w.push(np.ones((1, 30000, 2), np.uint8))
    w.flush()
    assert tape.take() == [f"ddc_wide_stream_open({ddc_wide.IQ_U8},240000,[1.0, 2.0])", f"pan_stream_open({ddc_wide.IQ_U8},256,50,3,0,240000)",
                           "pan_stream_push((30000, 2),uint8,1)", f"ddc_wide_stream_push(d_ptr={PAN_BUF:#x},n=30000)", "pan_stream_read(0,2)",
                           "pan_stream_push((30000, 2),uint8,1)", f"ddc_wide_stream_push(d_ptr={PAN_BUF:#x},n=30000)", "pan_stream_read(2,2)"] + \
        ["ddc_wide_stream_push((20160, 2),uint8,128)"] * 2
    p = rx.panorama
    assert p is w.panorama and p["r_next"] == 4 and p["data"].shape == (3, 256) and (p["data"] == 2.0).all() and (p["stats"] == 3).all()
    assert p["row_seconds"] == 256 * 50 / 240000 and p["f_hz"][128] == 0.0 and w.panorama_time(2) == 15000.0 + 2 * 256 * 50 / 240000
    assert w.n_pushed == 60000


def test_wide_in_refuses_two_streams_with_panorama(tape):
    rx = trp.rx_of(max_frames=2, sample_rate=48000, iq=True, dial_offsets_hz=(1.0, 2.0), panorama=True)
    with pytest.raises(_lib.Ft8rxError, match="panorama: 2 streams"):
        rx.wide_in.push(np.ones((2, 5000, 2), np.int16))
    with pytest.raises(_lib.Ft8rxError, match="n_fft"):
        trp.rx_of(sample_rate=48000, panorama={"n_fft": 100})


def test_decode_stream_with_panorama_runs_the_one_shot_first(tape):
    rx = trp.rx_of(max_frames=1)
    tape.push(("test_08",))
    x = np.ones((240000, 2), np.int16)
    rx.decode_stream(x, 240000, iq=True, dial_offsets_hz=[5.0], panorama={"n_fft": 1024, "n_avg": 10})
    calls = tape.take()
    assert calls[0] == f"pan((240000, 2),{ddc_wide.IQ_I16},1024,10,d_ptr=None,n=None)" and calls[1].startswith("ddc_wide(") and "pan" not in "".join(calls[1:])
    assert rx.panorama["data"].shape == (23, 1024) and rx.panorama["r_next"] == 23 and rx.panorama["stats"] is None
    tape.push(("test_08",))
    rx.decode_stream(x, 240000, iq=True, dial_offsets_hz=[5.0])
    assert "pan" not in "".join(tape.take())
