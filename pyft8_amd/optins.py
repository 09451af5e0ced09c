"""Which opt-in steps refuse which, for the Python surface: the twin of csrc/optins.hpp (the six handle settings, same relation),
plus the Python consumers of a batch that cannot carry some of them.  Every refusal of a combination in receiver.py, distributed.py
and _lib.Handle.set_packed_output is a call of refuse(); argument-range checks stay where the arguments are read.
Adding an opt-in: DESIGN.md section 15."""

PACKED, MSG_TYPES, AP_CALLS, RECALL, WEAK, REPORTS = SETTINGS = ("packed", "msg_types", "ap_calls", "recall", "weak", "reports")
PASSES, ARRAYS, PACKED_GATHER, FT4 = CONSUMERS = ("passes", "decode_frames_arrays", "packed_gather", "ft4")

_FIVE = {MSG_TYPES, AP_CALLS, RECALL, WEAK, REPORTS}
# row -> (the name refusals use, what it cannot run with, a hint: one for the row, or one per other party)
TABLE = {
    PACKED: ("the packed output (set_packed_output)", _FIVE, None),
    MSG_TYPES: ("msg_types != 0", {PACKED, AP_CALLS, RECALL, WEAK}, None),
    AP_CALLS: ("my_call / dx_call (a-priori decoding)", {PACKED, MSG_TYPES, WEAK}, None),
    RECALL: ("recall", {PACKED, MSG_TYPES, WEAK}, None),
    WEAK: ("weak=True", {PACKED, MSG_TYPES, AP_CALLS, RECALL}, None),
    REPORTS: ("reports=True", {PACKED}, None),
    PASSES: ("passes > 1 (subtraction)", _FIVE,
             {REPORTS: "the later passes decode a residual whose spectrum the measurement does not have"}),
    ARRAYS: ("decode_frames_arrays", {MSG_TYPES, RECALL, REPORTS}, "its _lib.MESSAGE_DTYPE rows have no place for them; use decode_frames"),
    PACKED_GATHER: ("the packed multi-GPU path (PackedGather)", _FIVE, "decode with Receiver.decode_frames instead"),
    # FT4 decoding (csrc/optins.hpp FT4_ROW): BP and OSD on the demodulator's LLRs with the msg_types mask, nothing else
    FT4: ("FT4 decoding (decode_frames_ft4)", {PACKED, AP_CALLS, RECALL, WEAK, REPORTS}, None),
}


def active(cfg, ap_calls=(), recall=False):
    """The settings a config (or a handle's cfg; stand-ins may lack fields) has on, as a set.  ap_calls: a handle's current calls;
    recall: a recall list was given for this batch."""
    on = {MSG_TYPES: getattr(cfg, "msg_types", 0),
          AP_CALLS: getattr(cfg, "ap_my_call", None) or getattr(cfg, "ap_dx_call", None) or any(ap_calls or ()),
          RECALL: recall or getattr(cfg, "recall", False), WEAK: getattr(cfg, "weak", False), REPORTS: getattr(cfg, "reports", False)}
    return {k for k, v in on.items() if v}


def conflict(asked, act):
    """The first setting, in table order, that is in `act` and that `asked` cannot run with, or None."""
    return next((s for s in SETTINGS if s in act and s != asked and s in TABLE[asked][1]), None)


def refuse(asked, act):
    """Raise Ft8rxError("<asked> is not supported together with <active>[: hint]") if `asked` cannot run with a setting in `act`."""
    c = conflict(asked, act)
    if c is None:
        return
    from ._lib import Ft8rxError
    name, _, hint = TABLE[asked]
    if isinstance(hint, dict):
        hint = hint.get(c)
    raise Ft8rxError(f"{name} is not supported together with {TABLE[c][0]}" + (f": {hint}" if hint else ""))
