"""Host-side FT8 message layer: 77-bit payload -> text, call-hash table, frame packaging.

Behavioural contract = reference PyFT8/decoders.py:16-115 (unpack and friends), PyFT8/databases.py:8-26
(add_call_hashes) and PyFT8/receiver.py:51-66 (check_and_package).  The GPU decides *validity*
(csrc/ft8_dev.h: ft8_valid77); this module only renders strings and replays the hash-table side
effects in the reference's call order.  Written table-driven from the FT8 message layout.
"""
import time

from .ft8_tables import PFX1_MASK, PFX1_TRAP, PFX2_BITMAP
from .ft8_msg_tables import MULT, SECTIONS

A37 = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
A38 = A37 + "/"
A27 = " ABCDEFGHIJKLMNOPQRSTUVWXYZ"
NTOKENS, MAX22 = 2063592, 4194304
AP_NAMES = ("NoAP", "CQ", "RR73", "73", "RRR")
# ipass 7 (ft8rx_set_ap_calls): the patterns ap 5..10 with the operator's call MY and the DX station's call DX
AP_CALL_NAMES = ("MY ???", "MY DX ???", "CQ DX ???", "MY DX RRR", "MY DX 73", "MY DX RR73")


# ipass 8 (ft8rx_set_recall): the hypothesis classes, the record's ap field
RECALL_CLASSES = ("repeat", "RRR", "RR73", "73", "report", "R-report")


def ap_name(ap):
    """The record's ap field -> the pattern's name (the reference's five, then the ipass-7 ones)."""
    return AP_NAMES[ap] if ap < 5 else AP_CALL_NAMES[ap - 5]


M64 = (1 << 64) - 1


class CallHashes:
    """(hash, nbits) -> callsign, nbits in {10, 12, 22}; last writer wins (databases.py:8-26)."""

    def __init__(self):
        self.by_hash = {}
        self.by_call = {}

    def clear(self):
        self.by_hash.clear()
        self.by_call.clear()

    def add(self, call):
        acc = 0
        for ch in (call + " " * 11)[:11]:
            acc = (acc * 38 + A38.find(ch)) & M64
        acc = (acc * 47055833459) & M64
        hs = [(acc >> (64 - nb), nb) for nb in (10, 12, 22)]
        for key in hs:
            self.by_hash[key] = call
        self.by_call[call] = hs

    def lookup(self, h, nb):
        return self.by_hash.get((h, nb), "...")


def _plausible(call):
    """decoders.py:107-115 without the file append."""
    if " " in call or len(call) < 3:
        return False
    a, b, c = call[0], call[1], call[2]
    if "A" <= a <= "Z" and (PFX1_MASK >> (ord(a) - 65)) & 1 and b.isdigit():
        if not ((PFX1_TRAP >> (ord(a) - 65)) & 1 and c.isdigit()):
            return True
    ia, ib = A37.find(a) - 1, A37.find(b) - 1
    return ia >= 0 and ib >= 0 and (PFX2_BITMAP[ia] >> ib) & 1 == 1 and c.isdigit()


def _call28_text(n28):
    v = n28 - NTOKENS - MAX22
    if v < 0:
        return "ZZ9ZZZ"          # python divmod / negative-index artefact of the reference at n28 = 6257895
    out = []
    for alphabet, size in ((A37, 37), (A37[1:], 36), ("0123456789", 10), (A27, 27), (A27, 27), (A27, 27))[::-1]:
        v, r = divmod(v, size)
        out.append(alphabet[r])
    return "".join(reversed(out)).strip()


def _field29(v29, i3, table):
    flag, n28 = v29 & 1, v29 >> 1
    if n28 < 3:
        return ("DE", "QRZ", "CQ")[n28]
    if n28 < 1004:
        return "CQ %03d" % (n28 - 3)
    if n28 < 21443:
        v, s = n28 - 1003, ""
        for _ in range(4):
            v, r = divmod(v, 27)
            s = A27[r] + s
        return "CQ " + s.strip()
    if n28 < NTOKENS + MAX22 - 1:
        return "<%s>" % table.lookup(n28 - NTOKENS, 22)
    call = _call28_text(n28)
    if not _plausible(call):
        return None
    if flag:
        call += "/P" if i3 == 2 else "/R"
        if call.endswith("/R") and call[0] not in "AKNW":
            return None
    table.add(call)
    return call


def _grid_or_report(g16):
    g15 = g16 & 0x7FFF
    if g15 < 32400:
        q, r = divmod(g15, 1800)
        s, r = divmod(r, 100)
        return chr(65 + q) + chr(65 + s) + "%02d" % r
    if g15 <= 32404:
        return ("", "", "RRR", "RR73", "73")[g15 - 32400]
    return ("R" if g16 >> 15 else "") + "%+03d" % (g15 - 32435)


def unpack(bits77, table):
    """77-bit int -> (call_a, call_b, extra) or None; mutates `table` exactly like the reference."""
    if not bits77:
        return None
    i3 = bits77 & 7
    body = bits77 >> 3
    if i3 in (1, 2):
        g16, cb, ca = body & 0xFFFF, (body >> 16) & 0x1FFFFFFF, (body >> 45) & 0x1FFFFFFF
        if g16 & 0x7FFF == 0:
            return None
        extra = _grid_or_report(g16)
        a = _field29(ca, i3, table)
        b = _field29(cb, i3, table)
        if a is None or b is None or extra == "":
            return None
        return (a, b, extra)
    if i3 == 4:
        cq, rrr, swap = body & 1, (body >> 1) & 3, (body >> 3) & 1
        n58, h12 = (body >> 4) & ((1 << 58) - 1), (body >> 62) & 0xFFF
        if bool(cq) == bool(rrr):
            return None
        first = "CQ" if cq else "<%s>" % table.lookup(h12, 12)
        s = ""
        for _ in range(12):
            n58, r = divmod(n58, 38)
            s = A38[r] + s
        s = s.strip()
        table.add(s)
        pair = (s, first) if swap else (first, s)
        return pair + (("", "RRR", "RR73", "73")[rrr],)
    return None


# ---- opt-in message types (config msg_types; include/ft8rx.h FT8RX_MT_*).  Bit layouts: Franke, Somerville, Taylor, "The FT4 and FT8
# Communication Protocols", QEX 2020.  The reference renders none of these (decoders.py:16-49 returns None).
MT_FREE_TEXT, MT_DXPEDITION, MT_FIELD_DAY, MT_TELEMETRY, MT_RTTY_RU, MT_EU_VHF = 1, 2, 4, 8, 16, 32
MT_ALL = 63
A42 = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ+-./?"
LOC6 = 18 * 18 * 10 * 10 * 24 * 24


def _c28(n28, table):
    """A c28 field of the opt-in types: the i3 = 1 field rule without the suffix flag (standard calls enter the table)."""
    return _field29(n28 << 1, 1, table)


def _bits(v, pos, n):
    return (v >> pos) & ((1 << n) - 1)


def unpack_ext(bits77, table, mask):
    """unpack() with the opt-in message types of `mask`: -> (first, second, rest) or None.  mask = 0 and i3 = 1, 2, 4 are unpack().
    None exactly where the device gate (csrc/ft8_dev.h: ft8_valid77_ext) rejects the word outside OSD.  Both c28 fields are rendered
    (and enter the table) before any range check, as in host_messages.hpp."""
    i3, n3 = bits77 & 7, (bits77 >> 3) & 7
    if not mask or not bits77 or i3 in (1, 2, 4):
        return unpack(bits77, table)
    if i3 == 0:
        v71 = bits77 >> 6
        if n3 == 0:                                       # free text: 13 characters of A42, first character most significant
            if not mask & MT_FREE_TEXT or v71 >= 42 ** 13:
                return None
            s = ""
            for _ in range(13):
                v71, r = divmod(v71, 42)
                s = A42[r] + s
            return (s.strip(), "", "")
        if n3 == 5:                                       # telemetry: 18 hex digits, leading zeros dropped
            if not mask & MT_TELEMETRY or v71 == 0:
                return None
            return ("%X" % v71, "", "")
        if n3 == 1:                                       # DXpedition: c28 c28 h10 r5
            if not mask & MT_DXPEDITION:
                return None
            a, b = _c28(_bits(bits77, 49, 28), table), _c28(_bits(bits77, 21, 28), table)
            if a is None or b is None:
                return None
            return (a + " RR73;", b, "<%s> %+03d" % (table.lookup(_bits(bits77, 11, 10), 10), 2 * _bits(bits77, 6, 5) - 30))
        if n3 in (3, 4):                                  # ARRL Field Day: c28 c28 R1 n4 k3 s7
            if not mask & MT_FIELD_DAY:
                return None
            a, b = _c28(_bits(bits77, 49, 28), table), _c28(_bits(bits77, 21, 28), table)
            s7 = _bits(bits77, 6, 7)
            if a is None or b is None or not 1 <= s7 <= len(SECTIONS):
                return None
            ntx = _bits(bits77, 16, 4) + 1 + (16 if n3 == 4 else 0)
            return (a, b, "%s%d%s %s" % ("R " if _bits(bits77, 20, 1) else "", ntx, chr(65 + _bits(bits77, 13, 3)), SECTIONS[s7 - 1]))
        return None
    if i3 == 3:                                           # ARRL RTTY Roundup: t1 c28 c28 R1 r3 s13
        if not mask & MT_RTTY_RU:
            return None
        a, b = _c28(_bits(bits77, 48, 28), table), _c28(_bits(bits77, 20, 28), table)
        s13 = _bits(bits77, 3, 13)
        if a is None or b is None:
            return None
        if 1 <= s13 <= 7999:
            ex = "%04d" % s13
        elif 8001 <= s13 <= 8000 + len(MULT):
            ex = MULT[s13 - 8001]
        else:
            return None
        return (("TU; " if _bits(bits77, 76, 1) else "") + a, b,
                "%s5%d9 %s" % ("R " if _bits(bits77, 19, 1) else "", _bits(bits77, 16, 3) + 2, ex))
    if i3 == 5:                                           # EU VHF contest: h12 h22 R1 r3 s11 g25
        if not mask & MT_EU_VHF:
            return None
        g = _bits(bits77, 3, 25)
        if g >= LOC6:
            return None
        loc = ""
        for size, base in ((24, "A"), (24, "A"), (10, "0"), (10, "0"), (18, "A")):
            g, r = divmod(g, size)
            loc = chr(ord(base) + r) + loc
        loc = chr(65 + g) + loc
        return ("<%s>" % table.lookup(_bits(bits77, 65, 12), 12), "<%s>" % table.lookup(_bits(bits77, 43, 22), 22),
                "%s%02d%04d %s" % ("R " if _bits(bits77, 42, 1) else "", 52 + _bits(bits77, 39, 3), _bits(bits77, 28, 11), loc))
    return None


def valid77_ext(bits77, mask, osd=False):
    """The device predicate ft8_valid77_ext (csrc/ft8_dev.h) in Python: does unpack_ext render the word?  osd: the word comes from an
    OSD trial, where free text and telemetry are never accepted."""
    if osd and mask and (bits77 & 0x3F) in (0, 0x28):   # i3.n3 = 0.0 / 0.5
        return False
    return unpack_ext(bits77, CallHashes(), mask) is not None


def msg_type(bits77):
    """The type code of a 77-bit word as the message dict's "msg_type": "i3.n3" for i3 = 0, "i3" otherwise."""
    i3 = bits77 & 7
    return "0.%d" % ((bits77 >> 3) & 7) if i3 == 0 else str(i3)


def _msg_text(bits77, text):
    """A message's line (duplicate filter, ALL.TXT): " ".join(msg_tuple) for i3 = 1, 2, 4 (the reference's), the empty fields of free
    text and telemetry left out for the opt-in types."""
    if bits77 & 7 in (0, 3, 5):
        return " ".join(x for x in text if x) if not text[1] else " ".join(text)
    return " ".join(text)


def decode_notes(rec):
    """'{source}_{AP}_{method}' + tweaks, formatted as the reference does (receiver.py:42,57,121,126,133,162)."""
    fine = rec["ipass"] >= 2
    if rec["ipass"] == 8:
        return "fine_RECALL_" + RECALL_CLASSES[rec["ap"]], tweaks_str(rec)
    meth = ("GOOD91 ", "LDPC5", "LDPC20", "OSD", "LDPC20_OSD", "CODEWORD")[rec["method"]]
    ap = AP_NAMES[rec["ap"]] if rec["ap"] < 5 else AP_CALL_NAMES[rec["ap"] - 5].replace(" ", "_")
    return ("fine" if fine else "grid") + "_" + ap + "_" + meth, tweaks_str(rec)


def tweaks_str(rec):
    if rec["ipass"] >= 2:
        return " t:%+03d f:%+03d" % (rec["ttweak"], rec["ftweak"])
    return "t:%+03d f:%+03d" % (0, 0)


_LAST_IPASS = {2: 0, 3: 1, 4: 1}     # status -> last ladder step taken (STOP_GRID_SD, STOP_COSTAS, STOP_FINE_SD)


def package_frame(rec, count, events, n_events, cyclestart_string="", band=None, odd_even=0, table=None, on_message=None, mask=0,
                  ap=False, recall=None):
    """Replay one frame's candidate records in the reference's order (receiver.py:389-398):
    per round all live candidates advance one ipass in llr_sd-descending (stable) order; CRC-passing
    unpack() calls update the hash table as they happen; first sighting of a message text is emitted.
    Returns the list of message dicts (reference receiver.py:61-64 keys).  mask != 0: the opt-in message types are rendered too
    (unpack_ext) and every dict gains "msg_type".  ap = True (a handle with a-priori calls, ft8rx_set_ap_calls): every dict gains
    "ap", the name of the pattern that decoded it.  ipass-7 events sit at slot 2 * ap (BP, codeword test) / 2 * ap + 1 (OSD).
    recall = (records, count) of the frame's recall area (ft8rx_fetch_recall): after every ladder message, the accepted ipass-8
    words in entry order, unless the text was emitted already; every dict then gains "recall"."""
    table = table if table is not None else CallHashes()
    rec = rec[:count]
    n_ev = min(int(n_events), len(events))
    per = {}
    for e in events[:n_ev]:
        per.setdefault((int(e["cand"]), int(e["ipass"])), []).append((int(e["slot"]), int(e["seq"]), (int(e["msg_hi"]) << 64) | int(e["msg_lo"])))
    last = []
    for r in rec:
        st = int(r["status"])
        last.append(int(r["ipass"]) if st == 1 else _LAST_IPASS.get(st, 7))
    out, seen = [], set()
    for rnd in range(8):
        live = [i for i in range(len(rec)) if last[i] >= rnd]
        if rnd == 1:
            live.sort(key=lambda i: float(rec[i]["grid_sd"]), reverse=True)
        elif rnd >= 2:
            live.sort(key=lambda i: float(rec[i]["fine_sd"]), reverse=True)
        for i in live:
            r = rec[i]
            decoded_here = int(r["status"]) == 1 and int(r["ipass"]) == rnd
            stop_key = None
            if decoded_here:
                m = int(r["method"])
                slot = 2 * int(r["ap"]) + (1 if m == 3 else 0) if rnd == 7 else int(r["ap"]) + (5 if m == 4 else 0)
                seq = 0 if m == 0 else (int(r["n_its"]) + 1 if m in (1, 2) else int(r["n_its"]))
                stop_key = (slot, seq)
            text = None
            done = set()
            for slot, seq, bits in sorted(per.get((i, rnd), [])):
                if stop_key is not None and (slot, seq) > stop_key:
                    break
                if (slot, seq) in done:
                    continue
                done.add((slot, seq))
                res = unpack_ext(bits, table, mask)
                if stop_key == (slot, seq):
                    text = res
            if decoded_here:
                word = (int(r["msg_hi"]) << 64) | int(r["msg_lo"])
                if text is None:        # event log truncated: render at emit time
                    text = unpack_ext(word, table, mask)
                if text is None:
                    continue
                msg_text = _msg_text(word, text)
                if msg_text in seen:
                    continue
                seen.add(msg_text)
                fine = rnd >= 2
                tsec = int(r["h0_idx"]) / 25.0
                fHz = 3.125 * int(r["f0_idx"])
                if fine:
                    tsec = float(tsec + int(r["ttweak"]) / 200)
                    fHz = float(fHz + int(r["ftweak"]) / 16)
                snr = "%+03d" % int(r["snr_fine"] if fine else r["snr_grid"])
                notes, tw = decode_notes(r)
                m = {"band": band, "tsec": tsec, "fHz": fHz, "msg_tuple": text, "their_snr": snr,
                     "their_tx_cycle": odd_even,
                     "all_txt_format": f"{cyclestart_string} {snr} {(tsec - 0.6):4.1f} {fHz:4.0f} ~ {msg_text}",
                     "cyclestart_string": cyclestart_string, "decode_completed": time.time(), "tweaks": tw,
                     "decode_notes": notes + tw}
                if mask:
                    m["msg_type"] = msg_type(word)
                if ap:
                    m["ap"] = ap_name(int(r["ap"]))
                if recall is not None:
                    m["recall"] = False
                out.append(m)
                if on_message is not None:
                    on_message(m)
    if recall is not None:
        rrec, rcount = recall
        for r in rrec[:int(rcount)]:
            if int(r["ipass"]) != 8 or int(r["status"]) != 1:
                continue
            word = (int(r["msg_hi"]) << 64) | int(r["msg_lo"])
            text = unpack_ext(word, table, mask)
            if text is None:
                continue
            msg_text = _msg_text(word, text)
            if msg_text in seen:
                continue
            seen.add(msg_text)
            tsec = float(int(r["h0_idx"]) / 25.0 + int(r["ttweak"]) / 200)
            fHz = float(3.125 * int(r["f0_idx"]) + int(r["ftweak"]) / 16)
            snr = "%+03d" % int(r["snr_fine"])
            notes, tw = decode_notes(r)
            m = {"band": band, "tsec": tsec, "fHz": fHz, "msg_tuple": text, "their_snr": snr, "their_tx_cycle": odd_even,
                 "all_txt_format": f"{cyclestart_string} {snr} {(tsec - 0.6):4.1f} {fHz:4.0f} ~ {msg_text}",
                 "cyclestart_string": cyclestart_string, "decode_completed": time.time(), "tweaks": tw, "decode_notes": notes + tw}
            if mask:
                m["msg_type"] = msg_type(word)
            if ap:
                m["ap"] = AP_NAMES[0]
            m["recall"] = True
            out.append(m)
            if on_message is not None:
                on_message(m)
    return out


def report_dict(rp):
    """One ft8rx_report (_lib.REPORT_DTYPE) -> {"snr": dB in 2500 Hz, "fHz", "tsec"}, or None for a slot without a valid report."""
    fl = int(rp["flags"])
    if not fl & 1 or fl & 2:
        return None
    return {"snr": float(rp["snr_db"]), "fHz": float(rp["f_hz"]), "tsec": float(rp["t_sec"])}


def message_dicts(msgs, count, cyclestart_string="", band=None, odd_even=0, on_message=None, ap=False, recall=False, reports=None):
    """Rows of the native packager (ft8rx_package_batch, _lib.MESSAGE_DTYPE) -> the reference's message dicts
    (receiver.py:57-65).  Same formatting as package_frame above.  recall = True (ft8rx_package_batch_recall rows): every dict
    gains "recall", True for the ipass-8 messages.  reports (the frame's row of Handle.fetch_reports; ft8rx_set_reports): every dict
    gains "report", the measured {"snr", "fHz", "tsec"} of the message's candidate -- None where there is none (an invalid report, a
    recall message); the reference's keys stay as they are."""
    out = []
    now = time.time()
    rows = msgs[:min(int(count), len(msgs))]
    if len(rows) == 0:
        return out
    # whole columns to Python lists first: field access on numpy structured scalars costs more than everything else here
    cols = [rows[k].tolist() for k in ("f", "h0_idx", "f0_idx", "ttweak", "ftweak", "snr", "ipass", "method", "ap", "fine")]
    ext = "i3" in rows.dtype.names                   # rows of ft8rx_package_batch_ext (_lib.MESSAGE_EXT_DTYPE): the opt-in types
    types = list(zip(rows["i3"].tolist(), rows["n3"].tolist())) if ext else [None] * len(rows)
    cands = rows["cand"].tolist()
    if reports is not None:                          # whole columns again: one lookup per message below
        r_fl, r_snr, r_f, r_t = (reports[k].tolist() for k in ("flags", "snr_db", "f_hz", "t_sec"))
    for (f3, h0, f0, tt, ft, sn, ipass, method, ap_, fn, ty), ci in zip(zip(*cols, types), cands):
        text = tuple(x.decode() for x in f3)
        tsec = h0 / 25.0
        fHz = 3.125 * f0
        if fn:
            tsec = float(tsec + tt / 200)
            fHz = float(fHz + ft / 16)
        snr = "%+03d" % sn
        rec = {"ipass": ipass, "method": method, "ap": ap_, "ttweak": tt, "ftweak": ft}
        notes, tw = decode_notes(rec)
        line = _msg_text(ty[0] | (ty[1] << 3), text) if ext else " ".join(text)
        d = {"band": band, "tsec": tsec, "fHz": fHz, "msg_tuple": text, "their_snr": snr, "their_tx_cycle": odd_even,
             "all_txt_format": f"{cyclestart_string} {snr} {(tsec - 0.6):4.1f} {fHz:4.0f} ~ {line}",
             "cyclestart_string": cyclestart_string, "decode_completed": now, "tweaks": tw, "decode_notes": notes + tw}
        if ext:
            d["msg_type"] = msg_type(ty[0] | (ty[1] << 3))
        if ap:
            d["ap"] = ap_name(int(ap_)) if ipass != 8 else AP_NAMES[0]
        if recall:
            d["recall"] = ipass == 8
        if reports is not None:
            ok = ipass != 8 and 0 <= ci < len(r_fl) and r_fl[ci] & 3 == 1            # measured and valid (report_dict's rule)
            d["report"] = {"snr": r_snr[ci], "fHz": r_f[ci], "tsec": r_t[ci]} if ok else None
        out.append(d)
        if on_message is not None:
            on_message(d)
    return out
