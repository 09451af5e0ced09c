"""bench.py --dump-outputs (CPU): the message lists of a step written as float .npy files, only the valid messages of each frame, a fixed
seeded sample of frames when the whole would exceed the 64 MB bound."""
import importlib.util
import os

import numpy as np

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _messages(B, cap, seed):
    from pyft8_amd import _lib
    rng = np.random.default_rng(seed)
    msgs = np.zeros((B, cap), _lib.MESSAGE_DTYPE)
    msgs["f"] = rng.integers(32, 127, size=msgs["f"].shape + (16,), dtype=np.uint8).view("S16")[..., 0]
    for k in ("cand", "f0_idx", "h0_idx"):
        msgs[k] = rng.integers(0, 900, size=msgs.shape)
    msgs["snr"] = rng.integers(-24, 20, size=msgs.shape)
    counts = rng.integers(0, cap + 1, size=B).astype(np.int32)
    return msgs, counts


def _load(d, suffix=""):
    return {f[:-len(suffix + ".npy")]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(suffix + ".npy")}


def test_dump_writes_the_valid_messages_as_floats(tmp_path):
    bench = _bench()
    msgs, counts = _messages(12, 9, 1)
    n_frames, n_msgs = bench.dump_outputs(str(tmp_path), msgs, counts)
    assert n_frames == 12 and n_msgs == int(counts.sum())
    out = _load(str(tmp_path))
    assert set(out) == {"frame_index", "message_counts", "msg_text"} | {"msg_" + k for k in bench.DUMP_FIELDS}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert np.array_equal(out["frame_index"], np.arange(12)) and np.array_equal(out["message_counts"], counts)
    valid = np.concatenate([msgs[f, :counts[f]] for f in range(12)])
    for k in bench.DUMP_FIELDS:
        assert np.array_equal(out["msg_" + k], valid[k].astype(np.float64)), k
    text = out["msg_text"].astype(np.uint8).view("S16").reshape(-1, 3)
    assert np.array_equal(text, valid["f"])
    assert sum(a.nbytes for a in out.values()) <= bench.DUMP_LIMIT_BYTES


def test_dump_samples_frames_beyond_the_limit_the_same_way_every_time(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 20000)
    msgs, counts = _messages(64, 12, 2)
    a, b = tmp_path / "a", tmp_path / "b"
    n_frames, _ = bench.dump_outputs(str(a), msgs, counts, suffix=".rank1")
    bench.dump_outputs(str(b), msgs, counts, suffix=".rank1")
    out, again = _load(str(a), ".rank1"), _load(str(b), ".rank1")
    assert 0 < n_frames < 64 and len(out["frame_index"]) == n_frames
    assert all(np.array_equal(out[k], again[k]) for k in out)
    idx = out["frame_index"].astype(int)
    assert np.all(np.diff(idx) > 0) and np.array_equal(out["message_counts"], counts[idx])
    assert sum(v.nbytes for v in out.values()) <= 20000
    assert np.array_equal(out["msg_cand"], np.concatenate([msgs[f, :counts[f]]["cand"] for f in idx]).astype(np.float64))
