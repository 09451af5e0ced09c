"""Time the streaming down-converter (ft8rx_ddc_stream_*) on the GPU: 16 channels with random dials out of ONE
stream of random IQ int16 at 12 D kHz, pushed from host memory as a live source does.  Prints one JSON line, host-to-host milliseconds
(every timed call ends in ft8rx_sync):
  chunk    a push of a 40-ms chunk, and of a single sample (an "empty" push: the copy and the bookkeeping, no tile completes);
  cycle    a whole cycle (15 s) pushed in 1-s chunks, one sync at the end; beside it the one-shot on the same samples and dials, from
           device memory (ft8rx_ddc) and from host memory (ft8rx_ddc_host), and the frame part;
  frame    ft8rx_ddc_stream_frame of a complete cycle.
Run one part under `rocprofv3 --kernel-trace --stats` for the kernels' own times (tools/rocprof_summary.py reads the database; the
40-ms pushes and the 1-s pushes launch the same kernel, so profile `chunk` and `cycle` in runs of their own).
Usage: python tools/ddc_stream_measure.py D [all|chunk|cycle|frame] [reps]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyft8_amd import _lib, ddc  # noqa: E402

N_OUT = 16


def stats(ms):
    ms = sorted(ms)
    return {"min": round(ms[0], 4), "median": round(ms[len(ms) // 2], 4), "max": round(ms[-1], 4), "n": len(ms)}


def main():
    D = int(sys.argv[1])
    part = sys.argv[2] if len(sys.argv) > 2 else "all"
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    rate, n = 12000 * D, _lib.NSAMP * D
    rng = np.random.default_rng(1)
    x = rng.integers(-32768, 32768, size=(1, n, 2), dtype=np.int64).astype(np.int16)
    src = np.zeros(N_OUT, np.int32)
    f = np.ascontiguousarray(rng.uniform(-0.5 * rate, 0.5 * rate - 1.0, N_OUT))
    fm = np.zeros(N_OUT)
    h = _lib.Handle(device=0, max_frames=N_OUT)
    L = _lib.lib()
    out = {"D": D, "rate_hz": rate, "n_out": N_OUT, "part": part}

    def push(a, count):
        h._chk(L.ft8rx_ddc_stream_push(h._h, a.ctypes.data, count, 0, None), "ft8rx_ddc_stream_push")

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        h.sync()
        return 1e3 * (time.perf_counter() - t0)

    h.ddc_stream_open(ddc.IQ_I16, rate, 1, src, f)
    c40 = rate // 25
    chunks = [np.ascontiguousarray(x[:, k * c40:(k + 1) * c40]) for k in range(n // c40)]
    secs = [np.ascontiguousarray(x[:, k * rate:(k + 1) * rate]) for k in range(15)]
    if part in ("all", "chunk"):
        for a in chunks[:50]:                                                         # warm-up: two seconds of stream
            push(a, c40)
        h.sync()
        out["push_40ms_ms"] = stats([timed(lambda a=a: push(a, c40)) for a in chunks[50:50 + 250]])       # ten seconds of stream
        out["push_1_sample_ms"] = stats([timed(lambda: push(chunks[0], 1)) for _ in range(100)])
        out["chunk_ms"] = 40.0
    if part in ("all", "cycle", "frame"):
        def cycle():
            for a in secs:
                push(a, rate)
        timed(cycle)                                                                  # warm-up
        if part != "frame":
            out["cycle_in_1s_pushes_ms"] = stats([timed(cycle) for _ in range(reps)])
    if part in ("all", "cycle"):
        d_x = torch.from_numpy(x).to(torch.device("cuda", 0))
        torch.cuda.synchronize()

        def one_shot():
            h._chk(L.ft8rx_ddc(h._h, d_x.data_ptr(), ddc.IQ_I16, rate, 1, n, n, N_OUT, src.ctypes.data, f.ctypes.data, 1.0, None, None,
                               fm.ctypes.data), "ft8rx_ddc")

        def one_shot_host():
            h._chk(L.ft8rx_ddc_host(h._h, x.ctypes.data, ddc.IQ_I16, rate, 1, n, n, N_OUT, src.ctypes.data, f.ctypes.data, 1.0, fm.ctypes.data),
                   "ft8rx_ddc_host")
        timed(one_shot), timed(one_shot_host)
        out["one_shot_device_ms"] = stats([timed(one_shot) for _ in range(reps)])
        out["one_shot_host_ms"] = stats([timed(one_shot_host) for _ in range(reps)])
    if part in ("all", "cycle", "frame"):
        m = h.ddc_stream_info()["m_produced"]
        timed(lambda: h.ddc_stream_frame(m - _lib.NSAMP, _lib.NSAMP))
        out["frame_ms"] = stats([timed(lambda: h.ddc_stream_frame(m - _lib.NSAMP, _lib.NSAMP)) for _ in range(20)])
    h.ddc_stream_close()
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
