"""Opt-in message types on the GPU (config msg_types): the device gate ft8_valid77_ext against its Python model, a round trip of
frames carrying all six types, and the default mode left exactly as it was."""
import random
import re

import numpy as np
import pytest
import torch  # noqa: F401 -- imported before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib); later GPU tests use torch


from conftest import ROOT, load_golden
from pyft8_amd import _lib, synth
from pyft8_amd import messages as M
from pyft8_amd.receiver import Receiver, decode_frames, frames_from_wav

pytestmark = pytest.mark.gpu
ALL = M.MT_ALL
TYPE_BIT = {"0.0": 1, "0.1": 2, "0.3": 4, "0.4": 4, "0.5": 8, "3": 16, "5": 32}
NEW_TYPES = set(TYPE_BIT)


@pytest.fixture(scope="module")
def H():
    h = _lib.Handle(max_frames=1)
    yield h
    h.close()


def test_valid77_ext_matches_python_model(H):
    """ft8rx_valid77_ext equals messages.valid77_ext on 1 M random and structured words per mask value: 0, each single type, all.
    The gate of a type does not depend on the other bits of the mask, so the model is evaluated at mask = all and mask = 0 and the
    other masks follow from the word's type."""
    import test_message_types as T
    rng = random.Random(2026)
    words = T.random_words(rng, 1000000)
    v_all = np.array([M.valid77_ext(w, ALL) for w in words])
    v_0 = np.array([M.unpack(w, M.CallHashes()) is not None for w in words])
    ty = [M.msg_type(w) for w in words]
    bit = np.array([TYPE_BIT.get(t, 0) for t in ty])
    assert v_all.sum() > 300000 and (v_all & (bit != 0)).sum() > 150000
    for mask in (0, 1, 2, 4, 8, 16, 32, ALL):
        want = v_0 if mask == 0 else np.where(bit == 0, v_all, v_all & ((bit & mask) != 0))
        got = H.valid77_ext(words, mask).astype(bool)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (mask, [hex(words[i]) for i in bad[:5]])
    assert np.array_equal(H.valid77_ext(words[:100000], 0), H.valid77(words[:100000]))


# ------------------------------------------------------------------------------------------------ round trip
HASHED_ONLY = ("KH1/KH7Z", "VP2EXX/4", "G4ABC/P", "PA3XYZ/MM", "DL1ABC/QRP")       # never rendered by any other message: hash misses


def texts_of_all_types(rng, n_each=4):
    calls = ["K1ABC", "W9XYZ", "N0CALL", "VE3ABC", "G4XYZ", "DL1AA", "JA1XYZ", "K7RA", "W1AW", "AA9ZZ", "KB2QQ", "N5ABC"]
    out = []
    for k in range(n_each):
        a, b = rng.sample(calls, 2)
        out.append(rng.choice(["TNX BOB 73 ", "CQ TEST FN", "QRZ? 599 ", "GL ES 73 ", "HELLO/WORLD"]) + str(k))
        out.append(f"{a} RR73; {b} <{rng.choice(HASHED_ONLY)}> {2 * rng.randrange(32) - 30:+03d}")
        out.append(f"{a} {b} {'R ' if k % 2 else ''}{rng.choice((1, 3, 16, 17, 32))}{'ABCDEFGH'[rng.randrange(8)]} {rng.choice(('WI', 'EMA', 'DX', 'ONE'))}")
        out.append("%X" % rng.getrandbits(70 - 8 * k))
        out.append(f"{'TU; ' if k % 2 else ''}{a} {b} {'R ' if k > 1 else ''}5{rng.randrange(2, 10)}9 {rng.choice(('WI', 'NWT', '0013', '1234'))}")
        out.append(f"<{rng.choice(HASHED_ONLY)}> <{rng.choice(HASHED_ONLY)}> {'R ' if k % 2 else ''}5{rng.randrange(2, 10)}{rng.randrange(2048):04d} "
                   f"{rng.choice(('IO91NP', 'JO22AB', 'FN42HX', 'RR99XX', 'AA00AA'))}")
    return out


def expected(text):
    """What a receiver with a fresh call-hash table renders: hashed calls it never heard are <...>."""
    return re.sub(r"<[^>]*>", "<...>", text)


def truth_origins(index, n):
    """(f0, t0) of the signals synth.frame_from_words(index, n words) placed: its random draws, replayed."""
    rng = np.random.Generator(np.random.Philox(key=synth.SEED_BASE + 77000000 + int(index)))
    rng.standard_normal(synth.NFRAME)
    out = []
    for k in range(n):
        f0 = 300.0 + 2400.0 * (k + 0.5) / n + rng.uniform(-3.0, 3.0)
        t0 = 0.5 + rng.uniform(-0.3, 0.8)
        rng.uniform(0.0, 8.0)
        out.append((f0, t0))
    return out


@pytest.fixture(scope="module")
def round_trip():
    rng = random.Random(11)
    frames, sent = [], []
    for i in range(6):
        texts = texts_of_all_types(rng)
        rng.shuffle(texts)
        words = [synth.pack77_ext(t, msg_type="telemetry" if re.fullmatch(r"[0-9A-F]+", t) else None) for t in texts]
        sent.append((texts, words))
        frames.append(synth.frame_from_words(900 + i, words, snr_range=(0.0, 8.0)))
    # the hashed calls must stay misses: no call the frames carry shares a 10 / 12 / 22-bit hash with one of them
    t = M.CallHashes()
    for c in ("K1ABC", "W9XYZ", "N0CALL", "VE3ABC", "G4XYZ", "DL1AA", "JA1XYZ", "K7RA", "W1AW", "AA9ZZ", "KB2QQ", "N5ABC"):
        t.add(c)
    for c in HASHED_ONLY:
        assert all(t.lookup(x, nb) == "..." for x, nb in _hashes(c)), c
    return np.stack(frames), sent


def _hashes(call):
    t = M.CallHashes()
    t.add(call)
    return t.by_call[call]


def test_round_trip_all_types(round_trip):
    """Frames of 24 signals, four of each new type at 0 .. +8 dB: decode_frames(msg_types="all") returns exactly the transmitted
    texts, at the origin the decoder reports for any message (its search-grid convention puts tsec ~75 ms after and fHz ~1.9 Hz
    below the true start: include/ft8rx.h, ft8rx_subtract) within one bin (3.125 Hz) and one hop (40 ms)."""
    audio, sent = round_trip
    got = decode_frames(audio, msg_types="all")
    dflt = decode_frames(audio)
    for f, (texts, words) in enumerate(sent):
        types = {M.msg_type(w) for w in words}
        assert {"0.0", "0.1", "0.5", "3", "5"} <= types and types & {"0.3", "0.4"}
        lines = {m["all_txt_format"].split(" ~ ")[1]: m for m in got[f] if m["msg_type"] in NEW_TYPES}
        want = {expected(M._msg_text(w, M.unpack_ext(w, M.CallHashes(), ALL))): k for k, w in enumerate(words)}
        assert set(lines) == set(want), (sorted(set(want) - set(lines)), sorted(set(lines) - set(want)))
        # anything else is a standard message the default mode emits as well (a false decode of the reference's own rule)
        others = [m["all_txt_format"] for m in got[f] if m["msg_type"] not in NEW_TYPES]
        assert set(others) <= {m["all_txt_format"] for m in dflt[f]}, others
        origins = truth_origins(900 + f, len(words))
        for line, m in lines.items():
            f0, t0 = origins[want[line]]
            assert abs(m["fHz"] - (f0 - 1.9)) <= 3.125 and abs(m["tsec"] - (t0 + 0.075)) <= 0.04, (line, m["fHz"], f0, m["tsec"], t0)
            assert m["msg_type"] == M.msg_type(words[want[line]])
            if m["msg_type"] in ("0.0", "0.5"):
                assert "OSD" not in m["decode_notes"]
    rx = Receiver("", None, msg_types="all")
    try:
        one = rx.decode_frame(audio[0])
    finally:
        rx.close()
    assert [m["all_txt_format"] for m in one] == [m["all_txt_format"] for m in got[0]] and len(one) >= 24


def test_round_trip_default_emits_none(round_trip):
    """The same frames at the default (msg_types = 0, the reference's rule): none of the transmitted messages is emitted."""
    audio, sent = round_trip
    for f, msgs in enumerate(decode_frames(audio)):
        assert msgs == [] or all("msg_type" not in m for m in msgs)
        texts = {expected(t) for t in sent[f][0]}
        assert not texts & {" ".join(m["msg_tuple"]) for m in msgs}


# ------------------------------------------------------------------------------------------------ default mode untouched
def _arrays(audio, **kw):
    from pyft8_amd.receiver import config_from_kwargs
    h = _lib.Handle(config_from_kwargs(**kw) if kw else None, max_frames=len(audio))
    try:
        rec, cnt, ev, evc = h.decode_batch(audio)
    finally:
        h.close()
    return rec, cnt, ev, evc


def test_default_mode_byte_identical():
    """msg_types = 0 given explicitly is the default: records, events and messages byte-identical on the golden frames and on every
    cycle of test_08.wav / test_09.wav."""
    names = ["test_08", "test_09", "synth_000000", "synth_100000", "synth_200000"]
    audio = [load_golden(n)[0] for n in names]
    for wav in ("test_08.wav", "test_09.wav"):
        audio += list(frames_from_wav(f"{ROOT}/tests/golden/{wav}"))
    audio = np.stack(audio)
    a = _arrays(audio)
    b = _arrays(audio, msg_types=0)
    (ra, ca, ea, eca), (rb, cb, eb, ecb) = a, b
    assert np.array_equal(ca, cb) and np.array_equal(eca, ecb)
    for f in range(len(audio)):              # the written part; the event log in a canonical order (its slots are taken by atomics)
        assert ra[f, :ca[f]].tobytes() == rb[f, :cb[f]].tobytes()
        ne = min(int(eca[f]), _lib.EVENT_CAP)
        key = ["cand", "ipass", "slot", "seq"]
        assert np.sort(ea[f, :ne], order=key).tobytes() == np.sort(eb[f, :ne], order=key).tobytes()
    ma, ma_n = _lib.package_batch(*a)
    mb, mb_n = _lib.package_batch(*b)
    assert ma.tobytes() == mb.tobytes() and ma_n.tobytes() == mb_n.tobytes() and ma_n.sum() > 0
    d0 = decode_frames(audio)
    d1 = decode_frames(audio, msg_types=0)
    strip = lambda L: [[{k: v for k, v in m.items() if k != "decode_completed"} for m in f] for f in L]
    assert strip(d0) == strip(d1)
    assert all("msg_type" not in m for f in d0 for m in f)


def test_all_mode_keeps_every_default_message():
    """In "all" mode the messages of the two recordings contain every default-mode message (a CRC-valid word of a new type can end
    a candidate's ladder before the standard message it would have reached; none does here), and no free text or telemetry carries
    an OSD method."""
    audio = np.concatenate([frames_from_wav(f"{ROOT}/tests/golden/{w}") for w in ("test_08.wav", "test_09.wav")])
    d0 = decode_frames(audio)
    d1 = decode_frames(audio, msg_types="all")
    for f0, f1 in zip(d0, d1):
        assert {m["msg_tuple"] for m in f0} <= {m["msg_tuple"] for m in f1}
        for m in f1:
            if m["msg_type"] in ("0.0", "0.5"):
                assert "OSD" not in m["decode_notes"], m


def test_no_osd_free_text_on_noise():
    """Noise-only frames at default kwargs, "all" mode: whatever is emitted, no free text or telemetry comes from an OSD trial."""
    rng = np.random.default_rng(5)
    audio = np.clip(np.rint(rng.standard_normal((64, synth.NFRAME)) * 1000.0), -32768, 32767).astype(np.int16)
    rx = Receiver("", None, max_frames=64, msg_types="all")
    try:
        rec, cnt, ev, evc = rx._handle(64).decode_batch(audio)
    finally:
        rx.close()
    for f in range(64):
        for r in rec[f, :cnt[f]]:
            if r["status"] == _lib.ST_DECODED and r["method"] in (_lib.M_OSD, _lib.M_LDPC_B_OSD):
                w = (int(r["msg_hi"]) << 64) | int(r["msg_lo"])
                assert M.msg_type(w) not in ("0.0", "0.5")


def test_arrays_and_passes_refuse_msg_types():
    rx = Receiver("", None, msg_types="all")
    try:
        audio = np.zeros((1, synth.NFRAME), np.int16)
        with pytest.raises(_lib.Ft8rxError):
            rx.decode_frames(audio, passes=2)
        with pytest.raises(_lib.Ft8rxError):
            rx.decode_frames_arrays(audio)
        h = rx._handle(1)
        with pytest.raises(_lib.Ft8rxError, match="msg_types"):       # ft8rx_message rows cannot hold the new types
            h.decode_messages(audio)
        with pytest.raises(_lib.Ft8rxError, match="msg_types"):
            h.set_packed_output(1, 2, 1 << 20)
    finally:
        rx.close()
