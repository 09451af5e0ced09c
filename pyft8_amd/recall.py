"""Recall decoding of stations heard 30 s earlier (ipass 8, ft8rx_set_recall): the host side.

A station in a QSO keeps its parity, its audio frequency and its clock offset, and its next message is nearly predictable from its
last one.  A recall entry is a message decoded two cycles back in the same stream, with its grid position; the GPU step
(kernels/recall.hpp) runs a forced fine sync there and tests the entry's likely continuations against the LLRs of that grid.

This module builds entries (from native message rows or from message dicts, also those of another decoder), and holds the numpy twin
of the hypothesis list and of the scorer (k_recall_score), which the tests compare the kernel against."""
import re

import numpy as np

from . import _lib, synth
from . import messages as M

STD = M.NTOKENS + M.MAX22                 # the first c28 of a standard call
PAYSYM = list(range(7, 36)) + list(range(43, 72))


def _field(word, lo, n):
    return (word >> lo) & ((1 << n) - 1)


def kind(word):
    """1 = "A B X" (A a standard call), 2 = "CQ / QRZ / DE B X", 0 = the word does not qualify (not i3 = 1 / 2, a hashed or
    non-standard call, a CQ with a number or a directed CQ)."""
    if word & 7 not in (1, 2):
        return 0
    ca, cb = _field(word, 49, 28), _field(word, 20, 28)
    if cb < STD or not (ca < 3 or ca >= STD):
        return 0
    text = M.unpack(word, M.CallHashes())
    if text is None or any("<" in t for t in text):
        return 0
    return 2 if ca < 3 else 1


def hypotheses(word):
    """The hypothesis words of an entry, in the kernel's order: the word itself, then (A B X only) A B RRR / RR73 / 73, the reports
    -30 .. +30, the R-reports R-30 .. R+30, with the repeat's duplicate dropped.  -> (words, classes); [] for a word that does not
    qualify.  Classes: index into messages.RECALL_CLASSES."""
    k = kind(word)
    if not k:
        return [], []
    words, cls = [word], [0]
    if k == 1:
        base = word & ~(0xFFFF << 3)
        cand = [(32402, 0, 1), (32403, 0, 2), (32404, 0, 3)]
        cand += [(32435 + nn, 0, 4) for nn in range(-30, 31)] + [(32435 + nn, 1, 5) for nn in range(-30, 31)]
        for g15, r, c in cand:
            w = base | (g15 << 3) | (r << 18)
            if w != word:
                words.append(w)
                cls.append(c)
    return words, cls


def _entry(word, f0_idx, h0_idx, ttweak=0, ftweak=0):
    e = np.zeros((), _lib.RECALL_ENTRY_DTYPE)
    e["msg_lo"], e["msg_hi"] = word & ((1 << 64) - 1), word >> 64
    e["f0_idx"], e["h0_idx"], e["ttweak"], e["ftweak"] = f0_idx, h0_idx, ttweak, ftweak
    return e


def _pack(text):
    try:
        return synth.pack77(*text)
    except (ValueError, TypeError, IndexError):
        return None


def _keep(items, cfg):
    """(snr, entry) pairs -> the qualifying entries inside cfg's search range, the RECALL_MAX with the highest SNR (stable), in
    their original order."""
    ok = []
    for i, (snr, e) in enumerate(items):
        w = (int(e["msg_hi"]) << 64) | int(e["msg_lo"])
        if not kind(w):
            continue
        if cfg is not None and not (cfg.f0_lo <= int(e["f0_idx"]) < cfg.f0_hi and cfg.h0_lo <= int(e["h0_idx"]) < cfg.h0_hi):
            continue
        ok.append((snr, i, e))
    best = sorted(ok, key=lambda t: -t[0])[:_lib.RECALL_MAX]
    return np.array([e for _, _, e in sorted(best, key=lambda t: t[1])], _lib.RECALL_ENTRY_DTYPE).reshape(-1)


def entries_from_rows(rows, count, cfg=None):
    """Native message rows (_lib.MESSAGE_DTYPE, one frame) -> entries: the word packed from the text (i3 = 1 / 2 packer), the grid
    position and tweaks exactly as the row holds them.  Words that do not qualify are skipped silently; of the rest, the
    RECALL_MAX with the highest SNR are kept (and those outside cfg's search range dropped)."""
    items = []
    for r in rows[:int(count)]:
        text = tuple(x.decode() for x in r["f"])
        w = _pack(text)
        if w is None:
            continue
        items.append((int(r["snr"]), _entry(w, int(r["f0_idx"]), int(r["h0_idx"]), int(r["ttweak"]) if r["fine"] else 0,
                                            int(r["ftweak"]) if r["fine"] else 0)))
    return _keep(items, cfg)


_TW = re.compile(r"t:([+-]\d+) f:([+-]\d+)")


def entries_from_dicts(dicts, cfg=None):
    """Message dicts (one frame: this package's, or any decoder's with msg_tuple, fHz, tsec) -> entries.  Where the dict carries
    this package's "tweaks" they are taken off first, so a dict made from a record lands on that record's grid position; otherwise
    the nearest grid position (f0_idx = fHz / 3.125, h0_idx = tsec * 25).  Words that do not qualify are skipped silently; of the
    rest, the RECALL_MAX with the highest SNR are kept (and those outside cfg's search range dropped)."""
    items = []
    for d in dicts:
        w = _pack(tuple(d["msg_tuple"]))
        if w is None:
            continue
        tt = ft = 0
        m = _TW.search(d.get("tweaks", "") or "")
        if m:
            tt, ft = int(m.group(1)), int(m.group(2))
        f0 = int(round((float(d["fHz"]) - ft / 16) / 3.125))
        h0 = int(round((float(d["tsec"]) - tt / 200) * 25))
        try:
            snr = int(d.get("their_snr", 0))
        except (TypeError, ValueError):
            snr = 0
        items.append((snr, _entry(w, f0, h0, tt, ft)))
    return _keep(items, cfg)


def llr_from_grid(sgrid):
    """79 x 8 fine-grid magnitudes -> (llr[174] float32, sd, snr): the arithmetic of llr_from_p (the reference's _dB_to_llr)."""
    g = np.asarray(sgrid, np.float32).reshape(79, 8)
    with np.errstate(divide="ignore"):
        p = (np.float32(20.0) * np.log10(g[PAYSYM])).astype(np.float32)             # [58, 8]
    snr = int(np.clip(int(np.float32(p.max() - p.min()) - np.float32(58.0)), -24, 24))
    mx = lambda idx: p[:, idx].max(axis=1)
    la = mx([4, 5, 6, 7]) - mx([0, 1, 2, 3])
    lb = mx([2, 3, 4, 7]) - mx([0, 1, 5, 6])
    lc = mx([1, 2, 6, 7]) - mx([0, 3, 4, 5])
    llr = np.stack([la, lb, lc], axis=1).reshape(174).astype(np.float32)
    mean = np.float32(llr.sum(dtype=np.float32) / np.float32(174))
    var = np.float32((llr * llr).sum(dtype=np.float32) / np.float32(174)) - mean * mean
    sd = np.float32(np.sqrt(var))
    return (np.float32(2.83) * llr / sd).astype(np.float32), float(sd), snr


def score(sgrid, word, max_hd=_lib.RECALL_MAX_HD_DEFAULT, min_gap=_lib.RECALL_MIN_GAP_DEFAULT):
    """The numpy twin of k_recall_score for one entry word on one fine grid -> dict(word, cls, index, hd, hd2, D, D2, accept), or
    None when the word does not qualify or the grid gives no LLRs."""
    words, cls = hypotheses(word)
    if not words:
        return None
    llr, sd, _ = llr_from_grid(sgrid)
    if not (sd > 0) or not np.isfinite(sd):
        return None
    hard = llr > 0
    a = np.abs(llr).astype(np.float64)
    res = []
    for i, w in enumerate(words):
        cw = synth.encode174(w)
        bits = np.array([(cw >> (173 - v)) & 1 for v in range(174)], bool)
        dis = bits != hard
        res.append((float(a[dis].sum()), i, int(dis.sum())))
    order = sorted(res)
    D, i, hd = order[0]
    D2, _, hd2 = order[1] if len(order) > 1 else (-1.0, None, 174)
    return dict(word=words[i], cls=cls[i], index=i, hd=hd, hd2=hd2, D=D, D2=D2, accept=hd <= max_hd and hd2 - hd >= min_gap)
