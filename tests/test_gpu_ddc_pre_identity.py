"""The two input pre-stages (ft8rx_ddc_wide*, ft8rx_ddc_rat*; DESIGN.md sections 16.2 - 16.4) put out the bytes they put out before
their host paths were folded into one: tests/golden/ddc_pre_parent.json holds the SHA-256 of every case's int16 frames, float32 outputs,
complex64 intermediate samples and mixed dials, recorded by tools/ddc_pre_record.py on an MI355X with a build of the commit before that
change.  The cases (one-shot through both entries, streams cut into uneven pushes -- shorter and longer than the history, one that
completes nothing, one from device memory -- with the intermediate samples read back across push boundaries, and a one-shot after
streams on the same handle) are the recorder's, computed here once.  A mismatch is a change of the output, not a reason to record again."""
import importlib.util
import json
import os

import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "ddc_pre_parent.json")) as _f:
    WANT = json.load(_f)


@pytest.fixture(scope="module")
def got():
    spec = importlib.util.spec_from_file_location("ddc_pre_record", os.path.join(ROOT, "tools", "ddc_pre_record.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    assert sorted(c[0] for c in rec.CASES) == sorted(WANT)
    return rec.hashes()


@pytest.mark.parametrize("case", sorted(WANT))
def test_bytes_are_the_parents(got, case):
    for mode, want in WANT[case].items():
        for what, value in want.items():
            assert got[case][mode][what] == value, f"{case} {mode}: {what} differs from the recorded parent"
    assert sorted(got[case]) == sorted(WANT[case])


def test_the_cases_take_every_path():
    """what the recording itself says about the cases: every stream made its tiles, and where the stage decimates one push made nothing"""
    streams = {c: v["stream"] for c, v in WANT.items() if "stream" in v}
    assert len(streams) == 12 and all(s["m"] in (2016, 3024) for s in streams.values())
    assert all(s["quiet_push"] for c, s in streams.items() if c != "rat-44100-real")          # 44100 -> 48000: every input completes a sample
    assert WANT["after-stream-wide-240000-iq16"]["one-shot"]["frames"] != WANT["wide-240000-iq16"]["one-shot"]["frames"]      # its own input
