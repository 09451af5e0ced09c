"""Opt-in message types (config msg_types): the renderer (messages.unpack_ext), its C++ twin (ft8rx_package_batch_ext) and the
encoder (synth.pack77_ext), on the CPU.  The reference renders none of these types (decoders.py:16-49 returns None); the yardstick
is the FT8 protocol definition (Franke, Somerville, Taylor, "The FT4 and FT8 Communication Protocols", QEX 2020)."""
import random

import numpy as np
import pytest

from pyft8_amd import _lib, synth
from pyft8_amd import messages as M
from pyft8_amd.ft8_msg_tables import MULT, SECTIONS
from pyft8_amd.receiver import msg_types_mask

ALL = M.MT_ALL


def word(*fields):
    """Fields (value, width) from the most significant end -> the 77-bit word (the protocol's bit order: first field first)."""
    v, n = 0, 0
    for val, width in fields:
        assert 0 <= val < (1 << width), (val, width)
        v, n = (v << width) | val, n + width
    assert n == 77
    return v


def c28(call):
    return synth.pack_c28(call)


def table_with(*calls):
    t = M.CallHashes()
    for c in calls:
        t.add(c)
    return t


def h(call, nb):
    return dict((n, x) for x, n in table_with(call).by_call[call])[nb]


def b42(text13):
    v = 0
    for ch in text13:
        v = v * 42 + M.A42.index(ch)
    return v


# (hand-derived word, text, tuple, type).  Layouts, first field first: free text f71 n3 i3; DXpedition c28 c28 h10 r5 n3 i3; Field
# Day c28 c28 R1 n4 k3 s7 n3 i3; telemetry t71 n3 i3; RTTY RU t1 c28 c28 R1 r3 s13 i3; EU VHF h12 h22 R1 r3 s11 g25 i3.
HASHED = ("KH1/KH7Z", "PA3XYZ", "G4ABC")


def known_answers():
    K = []
    # free text: 13 characters right-aligned, base 42, first character most significant
    K.append((word((b42("TNX BOB 73 GL"), 71), (0, 3), (0, 3)), "TNX BOB 73 GL", ("TNX BOB 73 GL", "", ""), "0.0"))
    K.append((word((b42("         CQ?"[-13:].rjust(13)), 71), (0, 3), (0, 3)), "CQ?", ("CQ?", "", ""), "0.0"))
    # free text with leading AND trailing spaces in its 13 characters: rendered trimmed (pack77_ext right-aligns, a different word)
    K.append((word((b42("  HI THERE   "), 71), (0, 3), (0, 3)), None, ("HI THERE", "", ""), "0.0"))
    # DXpedition: report = 2 r5 - 30; r5 = 11 -> -08, r5 = 0 -> -30, r5 = 31 -> +32; h10 hit (KH1/KH7Z in the table)
    K.append((word((c28("K1ABC"), 28), (c28("W9XYZ"), 28), (h("KH1/KH7Z", 10), 10), (11, 5), (1, 3), (0, 3)),
              "K1ABC RR73; W9XYZ <KH1/KH7Z> -08", ("K1ABC RR73;", "W9XYZ", "<KH1/KH7Z> -08"), "0.1"))
    K.append((word((c28("K1ABC"), 28), (c28("W9XYZ"), 28), (h("KH1/KH7Z", 10), 10), (0, 5), (1, 3), (0, 3)),
              "K1ABC RR73; W9XYZ <KH1/KH7Z> -30", ("K1ABC RR73;", "W9XYZ", "<KH1/KH7Z> -30"), "0.1"))
    K.append((word((c28("K1ABC"), 28), (c28("W9XYZ"), 28), (h("KH1/KH7Z", 10), 10), (31, 5), (1, 3), (0, 3)),
              "K1ABC RR73; W9XYZ <KH1/KH7Z> +32", ("K1ABC RR73;", "W9XYZ", "<KH1/KH7Z> +32"), "0.1"))
    # ... a hash miss renders <...> (h10 = 0 is nobody's hash in this table)
    K.append((word((c28("K1ABC"), 28), (c28("W9XYZ"), 28), (0, 10), (15, 5), (1, 3), (0, 3)),
              None, ("K1ABC RR73;", "W9XYZ", "<...> +00"), "0.1"))
    # Field Day: transmitters = n4 + 1 (n3 = 3) or n4 + 17 (n3 = 4); class = 'A' + k3; section = SECTIONS[s7 - 1]
    wi, ema, dx = 1 + SECTIONS.index("WI"), 1 + SECTIONS.index("EMA"), 1 + SECTIONS.index("DX")
    K.append((word((c28("K1ABC"), 28), (c28("W9XYZ"), 28), (0, 1), (5, 4), (0, 3), (wi, 7), (3, 3), (0, 3)),
              "K1ABC W9XYZ 6A WI", ("K1ABC", "W9XYZ", "6A WI"), "0.3"))
    K.append((word((c28("K1ABC"), 28), (c28("W9XYZ"), 28), (0, 1), (0, 4), (7, 3), (1, 7), (3, 3), (0, 3)),
              "K1ABC W9XYZ 1H AB", ("K1ABC", "W9XYZ", "1H AB"), "0.3"))
    K.append((word((c28("K1ABC"), 28), (c28("W9XYZ"), 28), (1, 1), (15, 4), (2, 3), (dx, 7), (3, 3), (0, 3)),
              "K1ABC W9XYZ R 16C DX", ("K1ABC", "W9XYZ", "R 16C DX"), "0.3"))
    K.append((word((c28("K1ABC"), 28), (c28("W9XYZ"), 28), (1, 1), (0, 4), (1, 3), (ema, 7), (4, 3), (0, 3)),
              "K1ABC W9XYZ R 17B EMA", ("K1ABC", "W9XYZ", "R 17B EMA"), "0.4"))
    K.append((word((c28("K1ABC"), 28), (c28("W9XYZ"), 28), (0, 1), (15, 4), (0, 3), (len(SECTIONS), 7), (4, 3), (0, 3)),
              "K1ABC W9XYZ 32A " + SECTIONS[-1], ("K1ABC", "W9XYZ", "32A " + SECTIONS[-1]), "0.4"))
    # telemetry: the 71 bits as 18 hex digits, leading zeros dropped
    K.append((word((0x123456789ABCDEF012, 71), (5, 3), (0, 3)), "123456789ABCDEF012", ("123456789ABCDEF012", "", ""), "0.5"))
    K.append((word((0x00000000000000ABC0, 71), (5, 3), (0, 3)), None, ("ABC0", "", ""), "0.5"))
    # RTTY Roundup: report 5 (r3 + 2) 9; s13 = serial 1 .. 7999 (4 digits) or 8000 + 1 + index into MULT
    K.append((word((1, 1), (c28("K1ABC"), 28), (c28("W9XYZ"), 28), (0, 1), (5, 3), (8001 + MULT.index("WI"), 13), (3, 3)),
              "TU; K1ABC W9XYZ 579 WI", ("TU; K1ABC", "W9XYZ", "579 WI"), "3"))
    K.append((word((0, 1), (c28("K1ABC"), 28), (c28("W9XYZ"), 28), (0, 1), (5, 3), (13, 13), (3, 3)),
              "K1ABC W9XYZ 579 0013", ("K1ABC", "W9XYZ", "579 0013"), "3"))
    K.append((word((0, 1), (c28("K1ABC"), 28), (c28("W9XYZ"), 28), (1, 1), (0, 3), (7999, 13), (3, 3)),
              "K1ABC W9XYZ R 529 7999", ("K1ABC", "W9XYZ", "R 529 7999"), "3"))
    K.append((word((0, 1), (c28("K1ABC"), 28), (c28("W9XYZ"), 28), (0, 1), (7, 3), (8000 + len(MULT), 13), (3, 3)),
              "K1ABC W9XYZ 599 " + MULT[-1], ("K1ABC", "W9XYZ", "599 " + MULT[-1]), "3"))
    # EU VHF: report 52 + r3, serial s11 (4 digits), locator g25 = ((((l0 18 + l1) 10 + d2) 10 + d3) 24 + l4) 24 + l5
    io91np = ((((8 * 18 + 14) * 10 + 9) * 10 + 1) * 24 + 13) * 24 + 15
    K.append((word((h("PA3XYZ", 12), 12), (h("G4ABC", 22), 22), (1, 1), (7, 3), (3, 11), (io91np, 25), (5, 3)),
              "<PA3XYZ> <G4ABC> R 590003 IO91NP", ("<PA3XYZ>", "<G4ABC>", "R 590003 IO91NP"), "5"))
    K.append((word((0, 12), (0, 22), (0, 1), (0, 3), (2047, 11), (0, 25), (5, 3)),
              None, ("<...>", "<...>", "522047 AA00AA"), "5"))
    return K


@pytest.mark.parametrize("k", range(len(known_answers())))
def test_known_answers(k):
    w, text, tup, ty = known_answers()[k]
    t = table_with(*HASHED)
    assert M.unpack_ext(w, t, ALL) == tup
    assert M.msg_type(w) == ty
    if text is not None:
        assert M._msg_text(w, tup) == text
        assert synth.pack77_ext(text) == w
    # only its own type bit renders it
    bit = {"0.0": 1, "0.1": 2, "0.3": 4, "0.4": 4, "0.5": 8, "3": 16, "5": 32}[ty]
    assert M.unpack_ext(w, table_with(*HASHED), bit) == tup
    assert M.unpack_ext(w, table_with(*HASHED), ALL & ~bit) is None
    assert M.unpack_ext(w, table_with(*HASHED), 0) is None and M.unpack(w, table_with(*HASHED)) is None


def test_pack77_ext_forms():
    assert synth.pack77_ext("00000ABC", msg_type="telemetry") == word((0xABC, 71), (5, 3), (0, 3))
    assert synth.pack77_ext("ABC") == word((b42("ABC".rjust(13)), 71), (0, 3), (0, 3))
    assert M.unpack_ext(synth.pack77_ext("  TNX  BOB "), M.CallHashes(), ALL) == ("TNX BOB", "", "")
    for bad in ("THIS IS TOO LONG FOR FT8", "K1ABC RR73; W9XYZ <KH1/KH7Z> -07", "K1ABC W9XYZ 33A WI", "<...> <G4ABC> 590003 IO91NP"):
        with pytest.raises(ValueError):
            synth.pack77_ext(bad)


def test_new_calls_enter_the_table():
    """Every standard call the new types render is added to the call-hash table (as call_29 does for i3 = 1 / 2, decoders.py:90)."""
    t = M.CallHashes()
    M.unpack_ext(synth.pack77_ext("K1ABC W9XYZ R 17B EMA"), t, ALL)
    assert {"K1ABC", "W9XYZ"} <= set(t.by_call)
    w = word((h("W9XYZ", 12), 12), (h("K1ABC", 22), 22), (0, 1), (0, 3), (1, 11), (0, 25), (5, 3))
    assert M.unpack_ext(w, t, ALL)[:2] == ("<W9XYZ>", "<K1ABC>")


def test_rejected_types_stay_rejected():
    rng = random.Random(5)
    for _ in range(2000):
        body = rng.getrandbits(71)
        for n3 in (2, 6, 7):
            assert M.unpack_ext((body << 6) | (n3 << 3), M.CallHashes(), ALL) is None
        for i3 in (6, 7):
            assert M.unpack_ext((rng.getrandbits(74) << 3) | i3, M.CallHashes(), ALL) is None
    # range gates: free text >= 42^13, telemetry 0, Field Day section 0 / beyond the table, RTTY exchange 0 / 8000 / beyond MULT,
    # EU VHF locator beyond RR99XX
    assert M.unpack_ext(word((42 ** 13, 71), (0, 3), (0, 3)), M.CallHashes(), ALL) is None
    assert M.unpack_ext(word((42 ** 13 - 1, 71), (0, 3), (0, 3)), M.CallHashes(), ALL) is not None
    assert M.unpack_ext(word((0, 71), (5, 3), (0, 3)), M.CallHashes(), ALL) is None
    for s7 in (0, len(SECTIONS) + 1, 127):
        assert M.unpack_ext(word((c28("K1ABC"), 28), (c28("W9XYZ"), 28), (0, 1), (0, 4), (0, 3), (s7, 7), (3, 3), (0, 3)), M.CallHashes(), ALL) is None
    for s13 in (0, 8000, 8001 + len(MULT), 8191):
        assert M.unpack_ext(word((0, 1), (c28("K1ABC"), 28), (c28("W9XYZ"), 28), (0, 1), (0, 3), (s13, 13), (3, 3)), M.CallHashes(), ALL) is None
    assert M.unpack_ext(word((0, 12), (0, 22), (0, 1), (0, 3), (0, 11), (M.LOC6, 25), (5, 3)), M.CallHashes(), ALL) is None
    # a c28 that the reference's plausibility rule rejects rejects the message (here: '/R'-free implausible call 'QQ1QQQ'? -> pick by rule)
    bad = next(n for n in range(M.NTOKENS + M.MAX22, M.NTOKENS + M.MAX22 + 10 ** 6, 7919) if not M._plausible(M._call28_text(n)))
    assert M.unpack_ext(word((bad, 28), (c28("W9XYZ"), 28), (0, 10), (0, 5), (1, 3), (0, 3)), M.CallHashes(), ALL) is None


def test_config_layout_unchanged():
    """msg_types is a handle setting (ft8rx_set_msg_types), not a field of ft8rx_config: the struct callers bind keeps its 15 fields."""
    import ctypes
    assert ctypes.sizeof(_lib.Config) == 15 * 4 and "msg_types" not in {f[0] for f in _lib.Config._fields_}
    assert _lib.Config().msg_types == 0 and _lib.default_config(msg_types=5).msg_types == 5 and _lib.Config().msg_types == 0
    assert _lib.MESSAGE_EXT_DTYPE.itemsize == 112


def test_msg_types_kwarg():
    assert msg_types_mask("all") == ALL and msg_types_mask(0) == 0
    assert msg_types_mask({"free_text", "eu_vhf"}) == 33
    for bad in ("none", {"contest"}, 64, -1):
        with pytest.raises(_lib.Ft8rxError):
            msg_types_mask(bad)
    from pyft8_amd.receiver import config_from_kwargs
    assert config_from_kwargs().msg_types == 0 and _lib.default_config().msg_types == 0
    assert config_from_kwargs(msg_types={"rtty_ru", "field_day"}).msg_types == 20


# ------------------------------------------------------------------------------------------------ C++ twin (ft8rx_package_batch_ext)
def random_words(rng, n):
    """Random 77-bit words and structured ones of every type, c28 fields from a pool of standard calls and hash fields from the pool's
    hashes about half of the time (so that hash hits and misses both happen as the tables evolve)."""
    pool = [synth.random_call(np.random.default_rng(rng.getrandbits(32))) for _ in range(300)]
    pool = [c for c in pool if "/" not in c]
    hp = table_with(*pool)

    def cf():
        return c28(rng.choice(pool)) if rng.random() < 0.6 else rng.getrandbits(28)

    def hf(nb):
        return hp.by_call[rng.choice(pool)][(10, 12, 22).index(nb)][0] if rng.random() < 0.5 else rng.getrandbits(nb)
    out = []
    for _ in range(n):
        r = rng.random()
        if r < 0.3:
            out.append(rng.getrandbits(77))
            continue
        ty = rng.randrange(10)
        if ty == 0:
            out.append(word((rng.randrange(42 ** 13 + 10 ** 18), 71), (0, 3), (0, 3)))
        elif ty == 1:
            out.append(word((cf(), 28), (cf(), 28), (hf(10), 10), (rng.getrandbits(5), 5), (1, 3), (0, 3)))
        elif ty == 2:
            out.append(word((cf(), 28), (cf(), 28), (rng.getrandbits(1), 1), (rng.getrandbits(4), 4), (rng.getrandbits(3), 3),
                            (rng.randrange(len(SECTIONS) + 3), 7), (rng.choice((3, 4)), 3), (0, 3)))
        elif ty == 3:
            out.append(word((rng.getrandbits(71) >> rng.randrange(71), 71), (5, 3), (0, 3)))
        elif ty == 4:
            out.append(word((rng.getrandbits(1), 1), (cf(), 28), (cf(), 28), (rng.getrandbits(1), 1), (rng.getrandbits(3), 3),
                            (rng.choice((rng.randrange(8192), rng.randrange(7998, 8070))), 13), (3, 3)))
        elif ty == 5:
            out.append(word((hf(12), 12), (hf(22), 22), (rng.getrandbits(1), 1), (rng.getrandbits(3), 3), (rng.getrandbits(11), 11),
                            (rng.randrange(M.LOC6 + 1000), 25), (5, 3)))
        elif ty == 6:
            out.append(synth.pack77(rng.choice(pool), rng.choice(pool), rng.choice(("RRR", "RR73", "73", "-05", "R+03", "FN42"))))
        elif ty == 7:      # i3 = 4: a non-standard call enters the table, h12 of a pool call
            out.append((hf(12) << 65) | (rng.getrandbits(58) << 7) | (rng.getrandbits(4) << 3) | 4)
        else:
            out.append((rng.getrandbits(71) << 6) | (rng.choice((2, 6, 7)) << 3))
    return out


def frames_of(words, n_cand=200):
    """Records / events of frames that decode the given words (GOOD91 at ipass 0, emit order = candidate order) or only CALL unpack()
    on them (an event of a candidate that never decodes: hash-table side effects only), alternately."""
    B = (len(words) + n_cand - 1) // n_cand
    rec = np.zeros((B, n_cand), _lib.RECORD_DTYPE)
    ev = np.zeros((B, _lib.EVENT_CAP), _lib.EVENT_DTYPE)
    cnt = np.zeros(B, np.int32)
    evc = np.zeros(B, np.int32)
    for k, w in enumerate(words):
        f, i = divmod(k, n_cand)
        r = rec[f, i]
        r["f0_idx"], r["h0_idx"], r["grid_sd"], r["fine_sd"] = 100 + i, 10, 9.0, 9.0
        if i % 2 == 0 or evc[f] >= _lib.EVENT_CAP:
            r["status"], r["ipass"], r["method"], r["msg_lo"], r["msg_hi"] = _lib.ST_DECODED, 0, _lib.M_GOOD91, w & (2 ** 64 - 1), w >> 64
        else:
            r["status"] = _lib.ST_STOP_GRID_SD
            e = ev[f, evc[f]]
            e["msg_lo"], e["msg_hi"], e["cand"], e["ipass"], e["slot"], e["seq"] = w & (2 ** 64 - 1), w >> 64, i, 0, 0, 0
            evc[f] += 1
        cnt[f] = i + 1
    return rec, cnt, ev, evc


def rows_text(msgs, n):
    return [tuple(x.decode() for x in m["f"]) for m in msgs[:n]]


def test_cpp_matches_python_renderer():
    """ft8rx_package_batch_ext and messages.package_frame(mask=all) render the same messages from 300 000 random and structured
    words, one persistent call-hash table on each side that evolves over the frames."""
    rng = random.Random(77)
    words = random_words(rng, 300000)
    rec, cnt, ev, evc = frames_of(words)
    table = _lib.CallHashTable()
    msgs, mcnt = _lib.package_batch_ext(rec, cnt, ev, evc, ALL, table=table)
    pt = M.CallHashes()
    n_new = 0
    for f in range(len(cnt)):
        want = M.package_frame(rec[f], cnt[f], ev[f], evc[f], table=pt, mask=ALL)
        got = rows_text(msgs[f], mcnt[f])
        assert got == [m["msg_tuple"] for m in want], f
        assert [M.msg_type(int(m["i3"]) | (int(m["n3"]) << 3)) for m in msgs[f, :mcnt[f]]] == [m["msg_type"] for m in want]
        n_new += sum(m["msg_type"] not in ("1", "2", "4") for m in want)
    assert len(table) == len(pt.by_hash)
    assert n_new > 20000                                    # the structured words of the new types do render
    # every type renders, and hash hits happen on the new types
    d = M.message_dicts(msgs[0], mcnt[0])
    assert all("msg_type" in x for x in d)


def test_mask_zero_is_the_reference_layer():
    """mask = 0: ft8rx_package_batch_ext renders exactly what ft8rx_package_batch (and messages.package_frame / unpack) does."""
    rng = random.Random(3)
    words = random_words(rng, 40000)
    rec, cnt, ev, evc = frames_of(words)
    a, ac = _lib.package_batch(rec, cnt, ev, evc)
    b, bc = _lib.package_batch_ext(rec, cnt, ev, evc, 0)
    assert np.array_equal(ac, bc)
    for f in range(len(cnt)):
        ra, rb = a[f, :ac[f]], b[f, :bc[f]]
        assert rows_text(ra, ac[f]) == rows_text(rb, bc[f])
        for k in ("cand", "f0_idx", "h0_idx", "snr", "ipass", "ap", "method", "fine"):
            assert np.array_equal(ra[k], rb[k]), k
        want = M.package_frame(rec[f], cnt[f], ev[f], evc[f])
        assert [m["msg_tuple"] for m in want] == rows_text(ra, ac[f])
        assert all("msg_type" not in m for m in want)
    for w in words[:20000]:
        assert M.unpack_ext(w, M.CallHashes(), 0) == M.unpack(w, M.CallHashes())


def test_all_txt_line():
    """all_txt_format of the new types reads like a WSJT-X ALL.TXT line: the message text, no padding fields."""
    words = [synth.pack77_ext(t) for t in ("TNX BOB 73 GL", "TU; K1ABC W9XYZ 579 WI", "123456789ABCDEF012")]
    rec, cnt, ev, evc = frames_of(words, n_cand=8)
    rec["status"][:] = np.where(np.arange(8) < 3, _lib.ST_DECODED, 0)
    rec["ipass"][:] = 0
    for i, w in enumerate(words):
        rec[0, i]["msg_lo"], rec[0, i]["msg_hi"] = w & (2 ** 64 - 1), w >> 64
    evc[:] = 0
    msgs, mcnt = _lib.package_batch_ext(rec, cnt, ev, evc, ALL)
    d = M.message_dicts(msgs[0], mcnt[0], cyclestart_string="240101_000000")
    assert [x["all_txt_format"].split(" ~ ")[1] for x in d] == ["TNX BOB 73 GL", "TU; K1ABC W9XYZ 579 WI", "123456789ABCDEF012"]
    assert [x["msg_type"] for x in d] == ["0.0", "3", "0.5"]
    assert d[0]["msg_tuple"] == ("TNX BOB 73 GL", "", "")


def test_packed_path_refuses_msg_types():
    class FakeHandle:
        cfg = _lib.default_config(msg_types=ALL)
    from pyft8_amd import distributed
    with pytest.raises(_lib.Ft8rxError, match="msg_types"):
        distributed.PackedGather(FakeHandle(), 4)
