"""FT4 without a GPU: the protocol constants against their published checks, the transmit side round trip through
the message layer, the host tone encoder against the Python one, and the float64 twin of the front end (pyft8_amd/ft4.py) on a
6-signal frame and on noise.  The GPU is held to this twin in tests/test_gpu_ft4.py."""
import numpy as np

import ft4_cases as cases
from pyft8_amd import _lib, ft4, messages, synth


def test_constants():
    assert len(ft4.RVEC_BITS) == 77 and (ft4.RVEC << 3).to_bytes(10, "big").hex().upper() == "4A5E89B4B08A7955BE28"
    a, b, c, d = ft4.COSTAS4
    assert a == (0, 1, 3, 2) and b == tuple(x ^ 1 for x in a) and c == tuple(x ^ 2 for x in a) and d == tuple(x ^ 3 for x in a)
    t = ft4.tones105(synth.pack77("CQ", "K1ABC", "FN42"))
    assert len(t) == ft4.NSYM == 105 and t[0] == 0 and t[104] == 0
    assert [tuple(t[p:p + 4]) for p in (1, 34, 67, 100)] == [a, b, c, d] and ft4.SYNC_POS == (1, 34, 67, 100)
    assert len(ft4.DATA_POS) == 87 and sorted(set(range(105)) - set(ft4.DATA_POS)) == [0, 1, 2, 3, 4, 34, 35, 36, 37, 67, 68, 69, 70, 100, 101, 102, 103, 104]
    assert [ft4.GRAY4_INV[ft4.GRAY4[v]] for v in range(4)] == [0, 1, 2, 3] and sorted(ft4.GRAY4) == [0, 1, 2, 3]
    # neighbouring tones differ in one bit
    assert all(bin(ft4.GRAY4_INV[k] ^ ft4.GRAY4_INV[k + 1]).count("1") == 1 for k in range(3))
    assert ft4.NSPS * ft4.NSYM == 60480 and ft4.HOP * (ft4.ROWS - 1) + ft4.NFFT == ft4.NFRAME == _lib.FT4_NSAMP
    assert (ft4.ROWS, ft4.COLS) == (_lib.FT4_ROWS, _lib.FT4_COLS)


def test_round_trip_and_host_encoder():
    """tones -> bits -> XOR rvec -> unpack gives the text back; ft8rx_ft4_encode_tones (host) equals tones105"""
    rng = np.random.Generator(np.random.Philox(key=4))
    words, texts, masks = [], [], []
    for _ in range(50):
        m = synth.random_message(rng)
        words.append(synth.pack77(*m)); texts.append(" ".join(m)); masks.append(0)
    for name, text, w in cases.ext_words():
        words.append(w); texts.append(text); masks.append(_lib.MSG_TYPE_BITS[name])
    tones = [ft4.tones105(w) for w in words]
    for w, text, mask, t in zip(words, texts, masks, tones):
        back = ft4.tones_to_bits77(t)
        assert back == w
        table = messages.CallHashes()
        for call in ("KH1/KH7Z", "PA3XYZ", "G4ABC"):
            table.add(call)
        got = messages.unpack_ext(back, table, mask) if mask else messages.unpack(back, table)
        assert got is not None and messages._msg_text(back, got) == " ".join(text.split()), (text, got)
        # the scrambled word is what the CRC and the code cover
        cw = synth.encode174(w ^ ft4.RVEC)
        assert cw >> 97 == w ^ ft4.RVEC and synth.crc14(w ^ ft4.RVEC) == (cw >> 83) & 0x3FFF
    lo, hi = cases.split_words(words)
    assert np.array_equal(_lib.ft4_encode_tones(lo, hi), np.array(tones, np.uint8))


def test_waveform():
    t = ft4.tones105(synth.pack77("CQ", "K1ABC", "FN42"))
    w = ft4.tones_to_wave(t, 1000.0)
    assert len(w) == 60480 and abs(w).max() <= 1.0 and abs(w[:8]).max() < 1e-3 and abs(w[-8:]).max() < 1e-3
    # each symbol's energy sits at its tone: the rectangular DFT of symbol s peaks at tones[s]
    A = ft4.amplitudes(w, 96, 0, 0, 0)            # 96 x 10.41667 = 1000 Hz, start at sample 0
    assert list(A[1:104].argmax(axis=1)) == t[1:104]


def test_twin_on_the_six_signal_frame():
    """every planted signal is found within 36 samples and 2.7 Hz, its hard decisions have 0 errors, and the numpy BP returns its word"""
    x, truth = cases.six()
    found = ft4.decode_twin(x)
    assert len(truth) == 6 and all(-8.0 <= t["snr"] <= 5.0 and 0.1 <= t["t0"] <= 1.5 for t in truth)
    assert min(abs(a["f0"] - b["f0"]) for i, a in enumerate(truth) for b in truth[i + 1:]) >= 150.0
    words = set()
    for t in truth:
        c = min(found, key=lambda c: abs(c["f0"] * ft4.BIN_HZ - t["f0"]) + 1000.0 * abs(ft4.HOP * c["h0"] / ft4.FS - t["t0"]))
        dt = ft4.HOP * c["h0"] + ft4.DT_STEP * c["tt"] - int(round(t["t0"] * ft4.FS))
        df = c["f0"] * ft4.BIN_HZ + c["ft"] * ft4.DF_HZ - t["f0"]
        assert abs(dt) <= 36 and abs(df) <= 2.7, (t, dt, df)
        assert int(((c["llr"] > 0) != (cases.codeword_bits(t["word"]) > 0.5)).sum()) == 0
        assert c["word"] == t["word"]
        assert abs(c["snr"] - t["snr"]) <= 6                  # the report reads low by a few dB
        words.add(c["word"])
    assert {c["word"] for c in found if c["word"] is not None} == words == {t["word"] for t in truth}


def test_twin_on_noise():
    """the noise-only frame: the default threshold lets a few per-bin maxima through; none of them decodes"""
    found = ft4.decode_twin(cases.noise_frame())
    assert len(found) <= 5 and all(c["word"] is None for c in found)
    assert ft4.decode_twin(cases.zero_frame()) == []


def test_llr_and_snr_conventions():
    A = np.zeros((105, 4))
    assert not ft4.llr_from_amplitudes(A).any() and ft4.snr_from_amplitudes(A) == -24      # std = 0: all-zero LLRs, finite
    w = synth.pack77("CQ", "K1ABC", "FN42")
    t = ft4.tones105(w)
    for s, tone in enumerate(t):
        A[s, tone] = 1.0
    llr = ft4.llr_from_amplitudes(A)
    assert np.array_equal(llr > 0, cases.codeword_bits(w) > 0.5) and abs(np.std(llr) - ft4.LLR_SCALE) < 1e-12
    assert ft4.bp_decode(llr) == w
    assert ft4.slot_parity("240101_000000") == 0 and ft4.slot_parity("240101_000007.5") == 1 and ft4.slot_parity("240101_000015") == 0
    assert ft4.slot_parity("240101_000022.5") == 1 and ft4.slot_parity("") == 0


def test_ranges():
    assert ft4.freq_range_to_f0() == (2, 567) and ft4.time_range_to_h0() == (-42, 168)
    assert ft4.freq_range_to_f0((100, 3000)) == (10, 289) and ft4.freq_range_to_f0((0, 6000)) == (0, 571)
