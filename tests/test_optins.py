"""The opt-in compatibility table of the Python surface (pyft8_amd/optins.py) without a GPU: the six settings against the literal
truth table that tests/host_asan_driver.cpp holds csrc/optins.hpp to, the consumers' rows, and the wording of every refusal that
the receiver kwargs can reach."""
import types

import pytest

from pyft8_amd import _lib, optins
from pyft8_amd.receiver import config_from_kwargs, set_ap_calls_cfg, set_weak_cfg

# asker (row) refused while a setting (column) is on; both in the order packed output, msg_types, ap_calls, recall, weak, reports
REFUSED = [[0, 1, 1, 1, 1, 1],
           [1, 0, 1, 1, 1, 0],
           [1, 1, 0, 0, 1, 0],
           [1, 1, 0, 0, 1, 0],
           [1, 1, 1, 1, 0, 0],
           [1, 0, 0, 0, 0, 0]]


def test_settings_equal_the_literal_table():
    S = optins.SETTINGS
    assert S == (optins.PACKED, optins.MSG_TYPES, optins.AP_CALLS, optins.RECALL, optins.WEAK, optins.REPORTS) and len(S) == 6
    assert set(optins.TABLE) == set(S) | set(optins.CONSUMERS)
    for i, a in enumerate(S):
        assert optins.TABLE[a][1] <= set(S)
        for j, s in enumerate(S):
            assert (optins.conflict(a, {s}) == s) == bool(REFUSED[i][j]), (a, s)
            assert REFUSED[i][j] == REFUSED[j][i]
    # with everything on, the first excluded setting in table order is the one named
    assert [optins.conflict(a, set(S)) for a in S] == ["msg_types", "packed", "packed", "packed", "packed", "packed"]
    assert all(optins.conflict(a, set()) is None for a in optins.TABLE)


def test_consumers():
    five = set(optins.SETTINGS) - {optins.PACKED}
    assert optins.TABLE[optins.PASSES][1] == five and optins.TABLE[optins.PACKED_GATHER][1] == five
    assert optins.TABLE[optins.ARRAYS][1] == {optins.MSG_TYPES, optins.RECALL, optins.REPORTS}
    names = [row[0] for row in optins.TABLE.values()]
    assert len(set(names)) == len(names) and all(names)
    for asked in optins.TABLE:                       # every refusal names both parties, and the hint follows a colon
        for s in optins.TABLE[asked][1]:
            with pytest.raises(_lib.Ft8rxError) as e:
                optins.refuse(asked, {s})
            text = str(e.value)
            assert text.startswith(f"{optins.TABLE[asked][0]} is not supported together with {optins.TABLE[s][0]}"), text
    with pytest.raises(_lib.Ft8rxError, match="reports=True: the later passes decode a residual"):
        optins.refuse(optins.PASSES, {optins.REPORTS})
    with pytest.raises(_lib.Ft8rxError, match="use decode_frames"):
        optins.refuse(optins.ARRAYS, {optins.RECALL})
    with pytest.raises(_lib.Ft8rxError, match="decode with Receiver.decode_frames instead"):
        optins.refuse(optins.PACKED_GATHER, {optins.WEAK})
    optins.refuse(optins.AP_CALLS, {optins.RECALL, optins.REPORTS})      # ipass 7 + ipass 8 run together


def test_active():
    assert optins.active(config_from_kwargs()) == set()
    c = config_from_kwargs(my_call="K1ABC")
    c.reports = True
    assert optins.active(c) == {optins.AP_CALLS, optins.REPORTS}
    assert optins.active(c, recall=True) == {optins.AP_CALLS, optins.REPORTS, optins.RECALL}
    assert optins.active(config_from_kwargs(weak=True)) == {optins.WEAK}
    assert optins.active(config_from_kwargs(msg_types="all")) == {optins.MSG_TYPES}
    stand_in = types.SimpleNamespace(max_cands=200)                     # a handle stand-in without the settings' fields
    assert optins.active(stand_in) == set() and optins.active(stand_in, ap_calls=(None, "K1ABC")) == {optins.AP_CALLS}


N = {k: v[0] for k, v in optins.TABLE.items()}


@pytest.mark.parametrize("kw, asked, other", [
    (dict(weak=True, msg_types="all"), "weak", "msg_types"),
    (dict(weak=True, my_call="K1ABC"), "weak", "ap_calls"),
    (dict(weak=True, dx_call="K1ABC"), "weak", "ap_calls"),
    (dict(my_call="K1ABC", msg_types=1), "ap_calls", "msg_types"),
    (dict(dx_call="K1ABC", msg_types={"telemetry"}), "ap_calls", "msg_types"),
])
def test_kwarg_refusals_name_both_parties(kw, asked, other):
    with pytest.raises(_lib.Ft8rxError) as e:
        config_from_kwargs(**kw)
    assert str(e.value) == f"{N[asked]} is not supported together with {N[other]}"


def test_cfg_setters_refuse_in_either_order():
    c = config_from_kwargs(weak=True)
    with pytest.raises(_lib.Ft8rxError) as e:
        set_ap_calls_cfg(c, "K1ABC", None)
    assert str(e.value) == f"{N['ap_calls']} is not supported together with {N['weak']}"
    set_ap_calls_cfg(c, None, None)                                     # turning off is never refused
    c = config_from_kwargs(msg_types="all")
    with pytest.raises(_lib.Ft8rxError) as e:
        set_weak_cfg(c, True)
    assert str(e.value) == f"{N['weak']} is not supported together with {N['msg_types']}"
    set_weak_cfg(c, False)
