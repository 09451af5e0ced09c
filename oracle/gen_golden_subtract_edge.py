"""Golden of the oracle's refine = 2 on the edge frame of tests/subtract_cases.py, as commit 376f6fd computed it -- the commit before
ft8o_refine2_subtract was split into the scans and ft8o_refine2_subtract_at.  The split must not change a bit of what it returns
(tests/test_subtract_oracle.py::test_refine2_refactor_is_byte_identical).

    git checkout 376f6fd -- oracle/ft8_oracle.c oracle/ft8_oracle.h oracle/oracle.py      (the oracle of that commit)
    python oracle/gen_golden_subtract_edge.py        -> tests/golden/subtract_edge_refine2.npz

Holds the six refined origins (float64), the subtracted flags and the float32 residual of the whole frame.  Test infrastructure only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle as O  # noqa: E402
import subtract_cases as SC  # noqa: E402


def main():
    wf = SC.frames()[0].astype(np.float32)
    origins, done = [], []
    for tones, fHz, tsec in SC.signals()[0]:
        d, f, t = O.refine2_subtract(wf, tones, fHz, tsec, True)
        origins.append((f, t))
        done.append(d)
    path = os.path.join(ROOT, "tests", "golden", "subtract_edge_refine2.npz")
    np.savez_compressed(path, origins=np.array(origins, np.float64), done=np.array(done, np.uint8), residual=wf)
    print(origins, done)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
