"""Time the wide pre-decimator's stream (ft8rx_ddc_wide_stream_*) on the GPU: ONE stream of full-scale random
samples, pushed a second at a time from host memory as a live source does, into n_out channels with random dials.  Prints one JSON
line: host-to-host milliseconds per 1-s push (every timed push ends in ft8rx_sync; two pushes of warm-up, then `reps`), and the same
push from device memory, which leaves out the page-locked copy and the upload.
Run it under `rocprofv3 --kernel-trace --stats` for the kernels' own times (tools/rocprof_summary.py reads the database):
k_ddc_pre_stream is the pre-stage, k_ddc_stream the down-converter behind it.
Usage: python tools/ddc_wide_measure.py [adc|rtl|narrow] [reps]
  adc     64.8 MS/s real int16 -> 16 channels      rtl     2.4 MS/s IQ uint8 -> 4 channels      narrow  240 kHz IQ int16 -> 2 channels"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyft8_amd import _lib  # noqa: E402
from pyft8_amd import ddc_wide as dw  # noqa: E402

CASES = {"adc": (dw.REAL_I16, 64800000, 16), "rtl": (dw.IQ_U8, 2400000, 4), "narrow": (dw.IQ_I16, 240000, 2)}


def stats(ms):
    ms = sorted(ms)
    return {"min": round(ms[0], 4), "median": round(ms[len(ms) // 2], 4), "mean": round(sum(ms) / len(ms), 4), "max": round(ms[-1], 4), "n": len(ms)}


def main():
    case = sys.argv[1] if len(sys.argv) > 1 else "rtl"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    kind, rate, n_out = CASES[case]
    rng = np.random.default_rng(1)
    info = np.iinfo(dw._DTYPE[kind])
    x = rng.integers(info.min, info.max + 1, size=(rate, 2) if dw.is_iq(kind) else rate, dtype=np.int64).astype(dw._DTYPE[kind])
    f = np.ascontiguousarray(rng.uniform(-0.5 * rate, 0.5 * rate - 1.0, n_out))
    h = _lib.Handle(device=0, max_frames=n_out)
    L = _lib.lib()
    mid, r0 = dw.plan(rate)
    out = {"case": case, "kind": dw.KIND_NAMES[kind], "rate_hz": rate, "n_out": n_out, "rate_mid_hz": mid, "R0": r0, "taps": len(dw.taps(rate))}

    def timed(ptr, on_device):
        t0 = time.perf_counter()
        h._chk(L.ft8rx_ddc_wide_stream_push(h._h, ptr, rate, on_device, None), "ft8rx_ddc_wide_stream_push")
        h.sync()
        return 1e3 * (time.perf_counter() - t0)

    h.ddc_wide_stream_open(kind, rate, f)
    for _ in range(2):
        timed(x.ctypes.data, 0)
    out["push_1s_host_ms"] = stats([timed(x.ctypes.data, 0) for _ in range(reps)])
    d_x = torch.from_numpy(x).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    timed(d_x.data_ptr(), 1)
    out["push_1s_device_ms"] = stats([timed(d_x.data_ptr(), 1) for _ in range(reps)])
    out["m_produced"] = h.ddc_stream_info()["m_produced"]
    h.ddc_wide_stream_close()
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
