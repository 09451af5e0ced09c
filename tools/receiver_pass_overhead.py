"""Host overhead of Receiver.decode_frames_arrays, this tree against another checkout (GPU box):

    python tools/receiver_pass_overhead.py --compare /path/to/other/checkout [--runs 10] [--frames 256] [--first this]

Alternating fresh processes -- the other tree, this one, the other, ... -- each import their own pyft8_amd/ and load THIS tree's
library through FT8RX_LIB, so only the Python side differs.  A process decodes the bench.py config-1 recipe (the frames of
tools/multipass_profile.py) with passes=1 and passes=2 and reports the median of its calls; the figures printed at the end are, per
passes, the median over each tree's processes and the other tree's own spread (max - min).  profiles/receiver_pass_notes.md."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(root, frames, calls):
    sys.path.insert(0, root)
    from pyft8_amd.receiver import Receiver
    rx = Receiver("x", None)
    h = rx._handle(frames)
    h.synth_frames(h.staging_ptr(), 4242, frames, n_signals=50, snr_range=(-10.0, 10.0))
    audio = h.download_audio(h.staging_ptr(), frames)
    out = {}
    for passes in (1, 2):
        for _ in range(2):
            counts = rx.decode_frames_arrays(audio, passes=passes)[1]
        t = []
        for _ in range(calls):
            t0 = time.perf_counter()
            rx.decode_frames_arrays(audio, passes=passes)
            t.append(1e3 * (time.perf_counter() - t0))
        out[f"passes={passes}"] = {"ms": statistics.median(t), "messages": int(counts.sum())}
    rx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", help="the other checkout (its pyft8_amd/ is imported, this tree's library loaded)")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--first", choices=("other", "this"), default="other", help="which tree's process opens each pair")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.frames, a.calls)
    env = dict(os.environ, FT8RX_LIB=os.path.join(HERE, "pyft8_amd", "libft8rx.so"),
               FT8RX_LIB_WIDE=os.path.join(HERE, "pyft8_amd", "libft8rx_wide.so"))
    trees = {"other": os.path.abspath(a.compare), "this": HERE}
    if a.first == "this":
        trees = dict(reversed(trees.items()))
    got = {k: [] for k in trees}
    for run in range(a.runs):
        for k, root in trees.items():
            # a fresh process per measurement; a failure ends the whole comparison
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--frames", str(a.frames), "--calls", str(a.calls)],
                               env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"run {run} of {k} ({root}) failed with {r.returncode}:\n{r.stderr[-2000:]}")
            got[k].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(run, k, got[k][-1], flush=True)
    for key in ("passes=1", "passes=2"):
        ms = {k: [g[key]["ms"] for g in v] for k, v in got.items()}
        assert len({g[key]["messages"] for v in got.values() for g in v}) == 1, "the two trees decode different message counts"
        print(f"{key}: other median {statistics.median(ms['other']):.2f} ms (min {min(ms['other']):.2f}, max {max(ms['other']):.2f}, "
              f"spread {max(ms['other']) - min(ms['other']):.2f}), this median {statistics.median(ms['this']):.2f} ms "
              f"(min {min(ms['this']):.2f}, max {max(ms['this']):.2f}); {got['this'][0][key]['messages']} messages in {a.frames} frames")


if __name__ == "__main__":
    main()
