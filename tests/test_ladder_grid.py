"""ft8rx_set_ladder_grid without a GPU: declared in the header, exported by both builds, and the Python side's cap is the compiled one."""
import os
import re
import subprocess

from conftest import ROOT
from pyft8_amd import _lib


def test_header_exports_and_cap():
    h = open(os.path.join(ROOT, "include", "ft8rx.h")).read()
    assert re.search(r"^int\s+ft8rx_set_ladder_grid\(ft8rx_handle\* h, int cap\);", h, re.M)
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_WIDE):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bft8rx_set_ladder_grid\b", syms), path
    assert hasattr(_lib.lib(), "ft8rx_set_ladder_grid") and hasattr(_lib.lib(wide=True), "ft8rx_set_ladder_grid")
    src = open(os.path.join(ROOT, "pyft8_amd", "csrc", "ft8rx.hip")).read()
    cap = re.search(r"#define LADDER_GRID_CAP \((\d+) \* (\d+) \* (\d+)\)", src)
    assert int(cap.group(1)) * int(cap.group(2)) * int(cap.group(3)) == _lib.LADDER_GRID_CAP
    # the timing builds index a per-block table by block id: the run-time cap never exceeds its rows
    osd = open(os.path.join(ROOT, "pyft8_amd", "csrc", "kernels", "osd.hpp")).read()
    assert int(re.search(r"g_osd_t\[(\d+)\]\[10\]", osd).group(1)) >= _lib.LADDER_GRID_CAP
