"""Time the down-converter (ft8rx_ddc) on the GPU: n_out outputs from n_streams streams of random IQ int16 at
12 D kHz, generated on the device.  Prints one JSON line (host-to-host milliseconds per call, input bytes per second).  Run it under
`rocprofv3 --kernel-trace --stats` for the kernel's own time (tools/rocprof_summary.py reads the database).
Usage: python tools/ddc_measure.py D n_streams n_out [reps]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyft8_amd import _lib, ddc  # noqa: E402


def main():
    D, n_streams, n_out = (int(a) for a in sys.argv[1:4])
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    rate, n = 12000 * D, _lib.NSAMP * D
    dev = torch.device("cuda", 0)
    x = torch.randint(-32768, 32768, (n_streams, n, 2), dtype=torch.int16, device=dev)
    torch.cuda.synchronize(dev)
    h = _lib.Handle(device=0, max_frames=n_out)
    rng = np.random.default_rng(1)
    src = np.ascontiguousarray(rng.permutation(n_out) % n_streams, np.int32)          # outputs of one stream are not neighbours in the call
    f = np.ascontiguousarray(rng.uniform(-0.5 * rate, 0.5 * rate - 1.0, n_out))
    fm = np.zeros(n_out)
    L = _lib.lib()

    def call():
        h._chk(L.ft8rx_ddc(h._h, x.data_ptr(), ddc.IQ_I16, rate, n_streams, n, n, n_out, src.ctypes.data, f.ctypes.data, 1.0, None, None,
                           fm.ctypes.data), "ft8rx_ddc")
        h.sync()
    for _ in range(2):
        call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append(1e3 * (time.perf_counter() - t0))
    in_bytes = 4.0 * n_streams * n
    best = min(ms)
    print(json.dumps({"D": D, "rate_hz": rate, "n_streams": n_streams, "n_out": n_out, "ms_host_to_host": [round(m, 3) for m in ms],
                      "input_GB": round(in_bytes / 1e9, 3), "input_TB_per_s_at_best": round(in_bytes / (best * 1e-3) / 1e12, 3)}))
    h.close()


if __name__ == "__main__":
    main()
