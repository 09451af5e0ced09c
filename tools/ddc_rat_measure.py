"""Time the rational resampler's stream (ft8rx_ddc_rat_stream_*) on the GPU: ONE stream of full-scale random
samples, pushed a second at a time from host memory as a live source does, into n_out channels with random dials.  Prints one JSON
line: host-to-host milliseconds per 1-s push (every timed push ends in ft8rx_sync; two pushes of warm-up, then `reps`), and the same
push from device memory, which leaves out the page-locked copy and the upload.  17 pushes in all with the default reps.
Run it under `rocprofv3 --kernel-trace --stats` for the kernels' own times (tools/rocprof_summary.py reads the database):
k_ddc_rat_stream is the resampler, k_ddc_stream the down-converter behind it.
Usage: python tools/ddc_rat_measure.py [audio|rtl|hackrf] [reps]
  audio   44100 Hz real int16 -> 1 channel      rtl     2.048 MS/s IQ int8 -> 4 channels      hackrf  10 MS/s IQ int8 -> 8 channels"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyft8_amd import _lib  # noqa: E402
from pyft8_amd import ddc_rat as dr  # noqa: E402

CASES = {"audio": (dr.REAL_I16, 44100, 1), "rtl": (dr.IQ_I8, 2048000, 4), "hackrf": (dr.IQ_I8, 10000000, 8)}


def stats(ms):
    ms = sorted(ms)
    return {"min": round(ms[0], 4), "median": round(ms[len(ms) // 2], 4), "mean": round(sum(ms) / len(ms), 4), "max": round(ms[-1], 4), "n": len(ms)}


def main():
    case = sys.argv[1] if len(sys.argv) > 1 else "rtl"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    kind, rate, n_out = CASES[case]
    rng = np.random.default_rng(1)
    info = np.iinfo(dr._DTYPE[kind])
    x = rng.integers(info.min, info.max + 1, size=(rate, 2) if dr.is_iq(kind) else rate, dtype=np.int64).astype(dr._DTYPE[kind])
    f = np.ascontiguousarray(rng.uniform(-0.5 * rate, 0.5 * rate - 1.0, n_out))
    h = _lib.Handle(device=0, max_frames=n_out)
    L = _lib.lib()
    mid, l, m, n = dr.plan(rate)
    out = {"case": case, "kind": dr.KIND_NAMES[kind], "rate_hz": rate, "n_out": n_out, "rate_mid_hz": mid, "L": l, "M": m, "taps": n,
           "taps_per_output": -(-n // l)}

    def timed(ptr, on_device):
        t0 = time.perf_counter()
        h._chk(L.ft8rx_ddc_rat_stream_push(h._h, ptr, rate, on_device, None), "ft8rx_ddc_rat_stream_push")
        h.sync()
        return 1e3 * (time.perf_counter() - t0)

    h.ddc_rat_stream_open(kind, rate, f)
    for _ in range(2):
        timed(x.ctypes.data, 0)
    out["push_1s_host_ms"] = stats([timed(x.ctypes.data, 0) for _ in range(reps)])
    d_x = torch.from_numpy(x).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    timed(d_x.data_ptr(), 1)
    out["push_1s_device_ms"] = stats([timed(d_x.data_ptr(), 1) for _ in range(reps)])
    out["m_produced"] = h.ddc_stream_info()["m_produced"]
    h.ddc_rat_stream_close()
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
