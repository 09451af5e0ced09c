"""Record what the two input pre-stages (ft8rx_ddc_wide*, ft8rx_ddc_rat*) and the down-converter behind them
(ft8rx_ddc, ft8rx_ddc_stream_*) put out, as SHA-256 hashes of the raw bytes: int16 frames, float32 outputs, complex64 intermediate
samples and the mixed dials.  tests/golden/ddc_pre_parent.json holds the hashes of the commit before the two host paths were folded into
one (the wide-* / rat-* / after-stream-* cases up to the latter) and of the commit before the sample formats moved into one table (the
ddc-* cases and the two after them); tests/test_gpu_ddc_pre_identity.py recomputes them with hashes() below.  Only Handle.ddc*,
ddc_wide* / ddc_rat* and ddc_stream_read / _info are used, so the script runs on either side of those changes.
Inputs are numpy.random.default_rng(seed) samples; every case makes at most three 1008-sample output tiles of three channels, one dial
within 1 kHz of -rate / 2 (the f_mixed wrap).
Usage: python tools/ddc_pre_record.py [out.json]        (default: tests/golden/ddc_pre_parent.json)"""
import hashlib
import json
import os
import sys

import numpy as np
import torch  # noqa: F401 -- before libft8rx.so loads, so that torch's own HIP runtime serves both (_lib.lib)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyft8_amd import _lib  # noqa: E402
from pyft8_amd import ddc as dd  # noqa: E402
from pyft8_amd import ddc_rat as dr  # noqa: E402
from pyft8_amd import ddc_wide as dw  # noqa: E402

TILE = 1008
MODS = {"wide": dw, "rat": dr, "ddc": dd}
DDC_SRC = (1, 0, 1)                                     # the plain down-converter: two streams feed the three channels
# (name, module, kind, rate, modes, output tiles)
CASES = [
    ("wide-240000-iq16", "wide", dw.IQ_I16, 240000, ("one-shot", "stream"), 3),          # R0 = 5, full 16-output tiles
    ("wide-2400000-u8", "wide", dw.IQ_U8, 2400000, ("stream",), 3),                      # R0 = 25
    ("wide-64800000-real", "wide", dw.REAL_I16, 64800000, ("stream",), 2),               # R0 = 675, several tap pieces, tk < 16
    ("wide-240000-real", "wide", dw.REAL_I16, 240000, ("one-shot",), 3),                 # g0 = 2
    ("rat-44100-real", "rat", dr.REAL_I16, 44100, ("one-shot", "stream"), 3),            # lane regime, L = 160
    ("rat-2048000-u8", "rat", dr.IQ_U8, 2048000, ("stream",), 3),                        # lane regime, P = 60
    ("rat-249900-iq16", "rat", dr.IQ_I16, 249900, ("one-shot",), 3),                     # wave regime by table size, P = 33
    ("rat-10000000-i8", "rat", dr.IQ_I8, 10000000, ("stream",), 3),                      # wave regime, P = 1291, more than one piece
    ("rat-44100-f32", "rat", dr.REAL_F32, 44100, ("one-shot",), 3),                      # a kind the wide stage does not take
    ("after-stream-wide-240000-iq16", "wide", dw.IQ_I16, 240000, ("one-shot",), 3),      # the one-shot buffers after streams have come and gone
    # every sample format once through k_ddc and k_ddc_stream themselves, and the two pre-stage formats the cases above leave out
    ("ddc-24000-real16", "ddc", dd.REAL_I16, 24000, ("one-shot", "stream"), 3),          # D = 2: no stage 1
    ("ddc-12000-real32", "ddc", dd.REAL_F32, 12000, ("one-shot", "stream"), 3),          # D = 1
    ("ddc-48000-iq16", "ddc", dd.IQ_I16, 48000, ("one-shot", "stream"), 2),              # D = 4
    ("ddc-96000-iq32", "ddc", dd.IQ_F32, 96000, ("one-shot", "stream"), 3),              # D = 8
    ("wide-480000-i8", "wide", dw.IQ_I8, 480000, ("one-shot", "stream"), 2),             # R0 = 5 at rate_mid 96000
    ("rat-250000-iq32", "rat", dr.IQ_F32, 250000, ("one-shot", "stream"), 3),            # lane regime, P = 33
]


def dials(rate):
    return [-0.5 * rate + 400.0, 0.11 * rate, 0.5 * rate - 700.0]


def samples(mod, kind, n, seed):
    rng = np.random.default_rng(seed)
    dt = mod._DTYPE[kind]
    shape = (n, 2) if mod.is_iq(kind) else n
    if mod is dd:                                                                   # [n_streams][n]
        shape = (2, n, 2) if mod.is_iq(kind) else (2, n)
    if np.dtype(dt).kind == "f":
        return rng.uniform(-30000.0, 30000.0, shape).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max + 1, size=shape, dtype=np.int64).astype(dt)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def geometry(which, rate):
    """(H, done): samples of history the stream keeps, and done(n_end) = intermediate samples complete once n_end inputs are in"""
    if which == "wide":
        _, R0 = dw.plan(rate)
        N0 = len(dw.taps(rate))
        return N0 - 1 + R0, lambda n_end: max((n_end - 1 - (N0 - 1) // 2) // R0 + 1, 0) if n_end > (N0 - 1) // 2 else 0
    _, L, M, N = dr.plan(rate)
    return -(-N // L), lambda n_end: max((n_end * L - (N - 1) // 2 - 1) // M + 1, 0) if n_end * L > (N - 1) // 2 else 0


def one_shot(h, which, kind, rate, x):
    call = getattr(h, f"ddc_{which}")
    fm, y = call(x, kind, rate, dials(rate), gain=0.75, want_float=True)             # the device entry
    a = h.download_audio(h.staging_ptr(), 3)
    fm_host = call(x, kind, rate, dials(rate), gain=0.75)                           # the host entry
    return {"frames": digest(a), "f32": digest(y), "f_mixed": digest(fm), "host_frames": digest(h.download_audio(h.staging_ptr(), 3)),
            "host_f_mixed": digest(fm_host)}


def stream(h, which, kind, rate, x):
    """x in pushes of uneven length: longer than the history H; shorter than H so that the ring copy wraps; one sample that completes
    no intermediate sample (where rate_mid < rate); one from device memory; the rest.  Intermediate samples are read back across the
    first pushes' boundaries and across the device push's end."""
    push, read_mid = getattr(h, f"ddc_{which}_stream_push"), getattr(h, f"ddc_{which}_stream_read_mid")
    H, done = geometry(which, rate)
    r = H // 2
    second = H - 1
    if done(H + r + second + 1) != done(H + r + second):                           # 1 sample more completes something: one shorter
        second -= 1
    lens = [H + r, second, 1, len(x) // 3 + 11, len(x) // 7 + 3]
    assert second > H - r and sum(lens) < len(x), (which, rate, H, lens, len(x))
    quiet = done(sum(lens[:3])) == done(sum(lens[:2]))
    fm = getattr(h, f"ddc_{which}_stream_open")(kind, rate, dials(rate), keep_f32=True)
    out = {"f_mixed": digest(fm), "quiet_push": bool(quiet)}
    try:
        at = 0
        for i, n in enumerate(lens):
            push(x[at:at + n], device=(i == 3))
            at += n
        k3, k4 = done(sum(lens[:3])), done(sum(lens[:4]))
        out["mid_head"] = digest(read_mid(0, min(k3 + 8, 64)))
        out["mid_boundary"] = digest(read_mid(k4 - 16, 32))
        m = 0
        while at < len(x):
            n = min(len(x) - at, 2 * len(x) // 7 + 5)
            m = push(x[at:at + n])
            at += n
        a, y = h.ddc_stream_read(0, m, want_float=True)
        out.update({"m": int(m), "frames": digest(a), "f32": digest(y)})
    finally:
        getattr(h, f"ddc_{which}_stream_close")()
    return out


def ddc_one_shot(h, kind, rate, x):
    fm, y = h.ddc(x, kind, rate, DDC_SRC, dials(rate), gain=0.75, want_float=True)   # the device entry
    a = h.download_audio(h.staging_ptr(), 3)
    fm_host = h.ddc(x, kind, rate, DDC_SRC, dials(rate), gain=0.75)                 # the host entry
    return {"frames": digest(a), "f32": digest(y), "f_mixed": digest(fm), "host_frames": digest(h.download_audio(h.staging_ptr(), 3)),
            "host_f_mixed": digest(fm_host)}


def ddc_stream(h, kind, rate, x):
    """x (both streams alike) in pushes of uneven length, one of them a single sample that completes no tile"""
    n = x.shape[1]
    fm = h.ddc_stream_open(kind, rate, 2, DDC_SRC, dials(rate), gain=0.75, keep_f32=True)
    out = {"f_mixed": digest(fm)}
    try:
        at = m = 0
        for i, k in enumerate([n // 3 + 11, 1, n // 7 + 3, n]):
            k = min(k, n - at)
            before, m = m, h.ddc_stream_push(x[:, at:at + k])
            at += k
            if i == 1:
                out["quiet_push"] = bool(m == before)
        a, y = h.ddc_stream_read(0, m, want_float=True)
        out.update({"m": int(m), "frames": digest(a), "f32": digest(y)})
    finally:
        h.ddc_stream_close()
    return out


def hashes():
    """{case: {mode: {what: sha256}}} of every case, on one handle, in the order of CASES"""
    h = _lib.Handle(device=0, max_frames=3)
    out = {}
    try:
        for seed, (name, which, kind, rate, modes, tiles) in enumerate(CASES):
            mod = MODS[which]
            n = -(-(tiles * TILE + 160) * rate // 12000)                            # the tiles and the reach of the filters behind them
            x = samples(mod, kind, n, 0xDDC0 + seed)
            out[name] = {}
            if which == "ddc":
                out[name]["one-shot"] = ddc_one_shot(h, kind, rate, x[:, :n - 237])
                out[name]["stream"] = ddc_stream(h, kind, rate, x)
                continue
            if "one-shot" in modes:
                out[name]["one-shot"] = one_shot(h, which, kind, rate, x[:n - 1237])
            if "stream" in modes:
                out[name]["stream"] = stream(h, which, kind, rate, x)
    finally:
        h.close()
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ddc_pre_parent.json")
    got = hashes()
    with open(path, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(got, sort_keys=True))
