"""Test helpers: turn the oracle's whole-frame output into the product's record/event arrays."""
import numpy as np

import oracle as O
from pyft8_amd import _lib


def bits_equal(a, b):
    """Bitwise equality of float32 arrays; NaNs must sit at the same positions (their sign/payload bits are
    not compared: x86 generates 0xFFC00000 for 0/0, gfx950 0x7FC00000)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def records_from_oracle(r, max_cands=200):
    rec = np.zeros(max_cands, _lib.RECORD_DTYPE)
    for i, c in enumerate(r["cands"]):
        g = rec[i]
        g["msg_lo"], g["msg_hi"] = c.msg_lo, c.msg_hi
        g["score"], g["grid_sd"], g["fine_sd"] = c.score, c.grid_sd, c.fine_sd
        g["f0_idx"], g["h0_idx"] = c.f0_idx, c.h0_idx
        g["ttweak"], g["ftweak"], g["snr_grid"], g["snr_fine"] = c.ttweak, c.ftweak, c.snr_grid, c.snr_fine
        g["status"] = c.status
        g["ipass"] = c.ipass if c.ipass >= 0 else 255
        g["ap"], g["method"], g["n_its"], g["nsync"] = c.ap, c.method, c.n_its, c.nsync
    ev = np.zeros(max(1, len(r["events"])), _lib.EVENT_DTYPE)
    for i, e in enumerate(r["events"]):
        ev[i]["msg_lo"], ev[i]["msg_hi"] = e.msg_lo, e.msg_hi
        ev[i]["cand"], ev[i]["ipass"] = e.cand, e.ipass
        ev[i]["slot"], ev[i]["seq"], ev[i]["valid"] = (e.pad >> 16) & 0xff, e.pad & 0xffff, e.valid
    return rec, len(r["cands"]), ev, len(r["events"])


def oracle_frame(audio):
    return O.decode_frame(audio, O.default_config(**_lib.fft_plans()))


def check_frame(rec, cnt, ev, evc, audio, js, ocfg, decode=None):
    """One frame of a batch result against the oracle's whole-frame decode (decode: None = O.decode_frame as it is bound at the time of
    the call, or O.decode_frame_f32 for a float32 frame): the candidate list, every record field the outcome defines, the messages in
    emit order -- and, with js, the reference's golden message dicts.  -> number of messages"""
    from pyft8_amd import messages as M
    r = (decode or O.decode_frame)(audio, ocfg)
    n = int(cnt)
    assert n == len(r["cands"])
    for i, c in enumerate(r["cands"]):
        g = rec[i]
        assert (g["f0_idx"], g["h0_idx"]) == (c.f0_idx, c.h0_idx)
        assert np.float32(g["score"]) == np.float32(c.score)
        assert int(g["status"]) == c.status, (i, int(g["status"]), c.status)
        assert np.float32(g["grid_sd"]) == np.float32(c.grid_sd) and g["snr_grid"] == c.snr_grid
        if c.status in (1, 4, 5) and (c.status != 1 or c.ipass >= 2):
            assert (g["ttweak"], g["ftweak"], g["nsync"]) == (c.ttweak, c.ftweak, c.nsync)
            assert np.float32(g["fine_sd"]) == np.float32(c.fine_sd) and g["snr_fine"] == c.snr_fine
        if c.status == 1:
            assert (int(g["ipass"]), int(g["ap"]), int(g["method"]), int(g["n_its"])) == (c.ipass, c.ap, c.method, c.n_its), i
            assert (int(g["msg_lo"]), int(g["msg_hi"])) == (c.msg_lo, c.msg_hi)
    msgs = M.package_frame(rec, n, ev, int(evc), cyclestart_string="700101_000015")
    o_txt = [" ".join(m["msg_tuple"]) for m in r["msgs"]]
    g_txt = [" ".join(m["msg_tuple"]) for m in msgs]
    assert g_txt == o_txt
    if js is not None:
        assert g_txt == [" ".join(m["msg_tuple"]) for m in js["messages"]]
        for m, ref in zip(msgs, js["messages"]):
            for key in ("tsec", "fHz", "their_snr", "all_txt_format", "tweaks", "decode_notes", "cyclestart_string", "their_tx_cycle"):
                assert m[key] == ref[key], (key, m[key], ref[key])
            assert list(m["msg_tuple"]) == ref["msg_tuple"]
    return len(g_txt)


# ---- OSD: which 91 columns form the most reliable basis (kernels/osd.hpp: osd_eliminate), as plain Python on 91-bit integers
def _g0_columns():
    """The 174 columns of G0 = [I | A^T]: bit r of column v = its entry in row r."""
    from pyft8_amd import synth
    return [1 << v for v in range(91)] + [sum(((g >> (90 - r)) & 1) << r for r in range(91)) for g in synth._GEN]


def _pivot(cols, p, b):
    """Make column p the unit vector of its row bit b: add that row to every other row in which column p has a 1."""
    m = cols[p] & ~b
    for q in range(174):
        if cols[q] & b:
            cols[q] ^= m


def osd_info_set_plain(order):
    """The reference's greedy loop (decoders.py:228-242): the positions in order, a column with a 1 in an unlocked row is accepted
    and pivots on the lowest such row, until 91 are accepted -> the accepted columns in that order."""
    cols, locked, basis = _g0_columns(), 0, []
    for v in (int(v) for v in order):
        a = cols[v] & ~locked
        if a and len(basis) < 91:
            b = a & -a
            _pivot(cols, v, b)
            locked |= b
            basis.append(v)
    return basis


def osd_info_set_novisit(order, ntriv_positions=96):
    """The kernel's rule: systematic columns at positions < 96 ("trivial") are not visited and their rows are reserved; a visited
    column pivots outside the locked and reserved rows, or steals the lowest row it has among the still-trivial columns after it
    (the robbed column goes back on the visit list), or is dependent; the basis is complete when accepted + trivial positions
    passed reach 91 -> (the basis columns by position, number of steals, number of dependent columns)."""
    order = [int(v) for v in order]
    cols = _g0_columns()
    triv = {p for p in range(ntriv_positions) if order[p] < 91}
    posrow = {order[p]: p for p in range(174) if order[p] < 91}
    lock_u = sum(1 << order[p] for p in triv)                     # locked by a pivot, or reserved for a trivial column
    visit = sorted(set(range(174)) - triv)
    accepted, steals, dependent = [], 0, 0
    while visit:
        p = visit.pop(0)
        if len(accepted) + sum(1 for t in triv if t < p) >= 91:
            break
        c = cols[order[p]]
        a = c & ~lock_u
        if not a:
            a = c & sum(1 << order[t] for t in triv if t > p)
            if not a:
                dependent += 1
                continue
            steals += 1
            q = posrow[(a & -a).bit_length() - 1]
            triv.remove(q)
            visit = sorted(visit + [q])
        b = a & -a
        _pivot(cols, order[p], b)
        lock_u |= b
        accepted.append(p)
    basis = sorted(accepted + sorted(triv)[:91 - len(accepted)])
    return [order[p] for p in basis], steals, dependent


def osd_steal_vectors(seed=7):
    """72 LLR vectors for the raw-vector OSD entry, each a valid codeword (bit 1 = positive LLR) with seeded magnitudes: three
    families x 0 / 1 / 2 sign errors x 8.  parity-first: the parity columns 91 .. 173 in [4, 8), the systematic ones in [0.5, 2) -- the
    basis starts with parity columns, many steals, and the decode depends on the whole reduced basis; mixed: 40 random systematic
    columns in [6, 8), the parity columns in [3, 5), the rest in [0.5, 2) -- no steal; random: everything in [0.5, 8).  The errors sit
    on members 79 .. 90 of the most reliable basis (the least reliable twelve: single flips 0 .. 11).
    -> [(family, errors, 77-bit word, float32[174])]"""
    from pyft8_amd import synth
    rng = np.random.default_rng(seed)
    out = []
    for family in ("parity-first", "mixed", "random"):
        for nerr in (0, 1, 2):
            for _ in range(8):
                word = synth.pack77(*synth.random_message(rng))
                cw = synth.encode174(word)
                if family == "parity-first":
                    mag = np.concatenate([rng.uniform(0.5, 2.0, 91), rng.uniform(4.0, 8.0, 83)])
                elif family == "mixed":
                    mag = np.concatenate([rng.uniform(0.5, 2.0, 91), rng.uniform(3.0, 5.0, 83)])
                    strong = rng.permutation(91)[:40]
                    mag[strong] = rng.uniform(6.0, 8.0, 40)
                else:
                    mag = rng.uniform(0.5, 8.0, 174)
                x = np.array([m if (cw >> (173 - v)) & 1 else -m for v, m in enumerate(mag)], np.float32)
                basis = osd_info_set_plain(O.argsort_f32(-np.abs(x)))
                for v in rng.permutation(basis[79:])[:nerr]:
                    x[v] = -x[v]
                out.append((family, nerr, word, x))
    return out


def osd_steal_checks(vectors):
    """What the vectors of osd_steal_vectors are there for, checked on the host: the kernel's rule gives the plain loop's basis for
    every one of them; every parity-first vector has >= 5 steals, every mixed one none, some vector has a dependent column; the
    oracle decodes every vector at (91, 91) to the encoded word, the ones with errors at a trial index > 0."""
    any_dependent = False
    for family, nerr, word, x in vectors:
        order = O.argsort_f32(-np.abs(x))
        basis, steals, dependent = osd_info_set_novisit(order)
        assert basis == osd_info_set_plain(order), (family, nerr)
        assert family != "parity-first" or steals >= 5, (family, steals)
        assert family != "mixed" or steals == 0, (family, steals)
        any_dependent |= dependent > 0
        ok, bits, trial, cols = O.osd(x, 91, 91)
        assert ok and bits == word and (trial > 0) == (nerr > 0), (family, nerr, ok, trial)
        assert list(cols) == basis, (family, nerr)
    assert any_dependent
