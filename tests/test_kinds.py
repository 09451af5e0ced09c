"""The sample kinds are stated once (pyft8_amd/kinds.py): the numbers are the header's, and ddc, ddc_wide, ddc_rat
and blank_in show rows of the one table and take exactly the kinds their entries take.  No GPU needed."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from pyft8_amd import blank_in, ddc, ddc_rat, ddc_wide, kinds

ACCEPTED = {ddc: {0, 1, 2, 3}, ddc_wide: {16, 17, 18, 19}, ddc_rat: {0, 1, 2, 3, 18, 19}, blank_in: {0, 2, 16, 17, 18, 19}}
MODULES = sorted(ACCEPTED, key=lambda m: m.__name__)
SHORT = {"REAL_I16": "real int16", "REAL_F32": "real float32", "IQ_I16": "IQ int16", "IQ_F32": "IQ float32", "IQ_U8": "IQ uint8", "IQ_I8": "IQ int8"}


def test_numbers_are_the_headers():
    with open(os.path.join(ROOT, "include", "ft8rx.h")) as f:
        header = dict(re.findall(r"^#define (FT8RX_(?:DDC|WIDE)_(?:REAL|IQ)_\w+)\s+(\d+)", f.read(), re.M))
    ours = {"FT8RX_DDC_" + n: getattr(kinds, n) for n in ("REAL_I16", "REAL_F32", "IQ_I16", "IQ_F32")}
    ours.update({"FT8RX_" + n: getattr(kinds, n) for n in ("WIDE_REAL_I16", "WIDE_IQ_I16", "WIDE_IQ_U8", "WIDE_IQ_I8")})
    assert {k: int(v) for k, v in header.items()} == ours and len(set(ours.values())) == 8
    assert set(kinds.NAMES) == set(kinds.DTYPE) == set(kinds.COMPONENTS) == set(ours.values())


@pytest.mark.parametrize("mod", MODULES, ids=[m.__name__.split(".")[-1] for m in MODULES])
def test_a_module_shows_rows_of_the_table(mod):
    assert set(mod.KINDS) == ACCEPTED[mod] and len(mod.KINDS) == len(ACCEPTED[mod])
    assert set(mod._DTYPE) == set(mod.KIND_NAMES) == ACCEPTED[mod]
    for k in mod.KINDS:
        assert mod._DTYPE[k] is kinds.DTYPE[k] and mod.KIND_NAMES[k] == kinds.NAMES[k] and mod.is_iq(k) is kinds.is_iq(k)
    for name, text in SHORT.items():                            # a module's own short names are kinds it takes, of that format
        for n in (name, "WIDE_" + name):
            assert not hasattr(mod, n) or (getattr(mod, n) in mod.KINDS and kinds.NAMES[getattr(mod, n)] == text)
    for k in set(kinds.NAMES) - ACCEPTED[mod]:
        if mod is ddc:
            assert not mod.is_iq(k)
        else:
            with pytest.raises(mod._lib.Ft8rxError, match="kind"):
                mod.is_iq(k)


def test_bytes_shapes_and_thresholds():
    for k in kinds.NAMES:
        dt = np.dtype(kinds.DTYPE[k])
        assert kinds.sample_bytes(k) == dt.itemsize * kinds.COMPONENTS[k] == np.zeros(kinds.shape(k, 1), dt).nbytes
        assert kinds.is_iq(k) == (kinds.COMPONENTS[k] == 2) == kinds.NAMES[k].startswith("IQ") and kinds.is_integer(k) == (dt.kind in "iu")
        assert kinds.NAMES[k].endswith(dt.name)
    assert {k: kinds.sample_bytes(k) for k in sorted(kinds.NAMES)} == {0: 2, 1: 4, 2: 4, 3: 8, 16: 2, 17: 4, 18: 2, 19: 2}
    assert [int(256 * blank_in.threshold_default(k)) for k in blank_in.KINDS] == [2048, 1408, 2048, 1408, 1408, 1408]
    assert all(kinds.is_integer(k) for k in blank_in.KINDS)
