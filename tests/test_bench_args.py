"""bench.py's command line (CPU): a plain run leaves out everything beyond the headline, --full brings it back as it was."""
import importlib.util
import os

import pytest

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_has_no_keep_busy_steps():
    args, explicit = _bench().parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not args.full and args.min_seconds == 0.0 and (args.steps, args.warmup) == (20, 5)
    assert explicit == {"--gpus", "--steps", "--warmup"}


def test_full_run_keeps_the_former_defaults():
    args, _ = _bench().parse_args(["--full"])
    assert args.full and args.min_seconds == 3.0 and (args.steps, args.warmup, args.frames) == (100, 10, 256)
    assert not (args.no_cpu_baseline or args.no_host_entry or args.no_other_configs)


def test_explicit_min_seconds_and_presets_hold_either_way():
    bench = _bench()
    for extra in ([], ["--full"]):
        args, _ = bench.parse_args(["--min-seconds", "1.5"] + extra)
        assert args.min_seconds == 1.5
        args, _ = bench.parse_args(["--config", "2"] + extra)
        assert (args.frames, args.bp_iters, tuple(args.osd), args.steps, args.warmup) == (4096, 30, (30, 2), 3, 1)


def test_other_configs_needs_full():
    bench = _bench()
    with pytest.raises(SystemExit):
        bench.parse_args(["--other-configs"])
    assert bench.parse_args(["--other-configs", "--full"])[0].other_configs
