"""Time the spectrogram stage behind the streaming down-converter (ft8rx_ddc_stream_grid_*) on the GPU: the
pushes of tools/ddc_stream_measure.py -- 16 channels with random dials out of ONE stream of random IQ int16 at 12 D kHz, from host
memory -- with the grid off and on, in the same run.  Prints one JSON line, host-to-host milliseconds (every timed call ends in
ft8rx_sync):
  push_40ms    a push of a 40-ms chunk: a tile (1008 outputs) completes every 2.1 pushes, and with it 2 or 3 hops;
  push_1s      a push of a 1-s chunk: 25 hops complete per push;
  push_1s_read the same followed by ft8rx_ddc_stream_grid_read of the rows it completed, as the live layer does (grid on only);
  worst_fraction   the slowest push as a fraction of the chunk's duration -- real time is met below 1.
Run one part under `rocprofv3 --kernel-trace --stats` for k_grid_stream's own time (tools/rocprof_summary.py reads the database).
Usage: python tools/ddc_grid_measure.py D [all|off|on] [n_rows]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyft8_amd import _lib, ddc  # noqa: E402

N_OUT = 16


def stats(ms):
    ms = sorted(ms)
    return {"min": round(ms[0], 4), "median": round(ms[len(ms) // 2], 4), "max": round(ms[-1], 4), "n": len(ms)}


def main():
    D = int(sys.argv[1])
    part = sys.argv[2] if len(sys.argv) > 2 else "all"
    n_rows = int(sys.argv[3]) if len(sys.argv) > 3 else 750
    rate, n = 12000 * D, _lib.NSAMP * D
    rng = np.random.default_rng(1)
    x = rng.integers(-32768, 32768, size=(1, n, 2), dtype=np.int64).astype(np.int16)
    src = np.zeros(N_OUT, np.int32)
    f = np.ascontiguousarray(rng.uniform(-0.5 * rate, 0.5 * rate - 1.0, N_OUT))
    h = _lib.Handle(device=0, max_frames=N_OUT)
    L = _lib.lib()
    out = {"D": D, "rate_hz": rate, "n_out": N_OUT, "n_rows": n_rows, "part": part}
    c40 = rate // 25
    chunks = [np.ascontiguousarray(x[:, k * c40:(k + 1) * c40]) for k in range(n // c40)]
    secs = [np.ascontiguousarray(x[:, k * rate:(k + 1) * rate]) for k in range(15)]

    def push(a, count):
        h._chk(L.ft8rx_ddc_stream_push(h._h, a.ctypes.data, count, 0, None), "ft8rx_ddc_stream_push")

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        h.sync()
        return 1e3 * (time.perf_counter() - t0)

    def push_and_read(a, count, q):
        push(a, count)
        info = h.ddc_stream_grid_info()
        if info["q_next"] > q[0]:
            h.ddc_stream_grid_read(max(q[0], info["q_first_held"]), info["q_next"] - max(q[0], info["q_first_held"]))
        q[0] = info["q_next"]

    for grid in ([False, True] if part == "all" else [part == "on"]):
        key = "grid_on" if grid else "grid_off"
        h.ddc_stream_open(ddc.IQ_I16, rate, 1, src, f)
        if grid:
            h.ddc_stream_grid_open(137, n_rows)
        for a in chunks[:50]:                                                         # warm-up: two seconds of stream
            push(a, c40)
        h.sync()
        r = {"push_40ms_ms": stats([timed(lambda a=a: push(a, c40)) for a in chunks[50:50 + 250]])}       # ten seconds of stream
        for a in secs[:2]:
            push(a, rate)
        h.sync()
        r["push_1s_ms"] = stats([timed(lambda a=a: push(a, rate)) for a in secs[2:] + secs])
        if grid:
            q = [h.ddc_stream_grid_info()["q_next"]]
            r["push_40ms_read_ms"] = stats([timed(lambda a=a: push_and_read(a, c40, q)) for a in chunks[:250]])
            r["push_1s_read_ms"] = stats([timed(lambda a=a: push_and_read(a, rate, q)) for a in secs])
        r["worst_fraction_40ms"] = round(max(v["max"] for k, v in r.items() if k.startswith("push_40ms")) / 40.0, 4)
        r["worst_fraction_1s"] = round(max(v["max"] for k, v in r.items() if k.startswith("push_1s")) / 1000.0, 4)
        out[key] = r
        h.ddc_stream_close()
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
