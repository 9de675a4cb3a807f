"""CPU: bench.py's plain run measures the headline figure only; --full adds the CPU baseline, the clock probe and the other
configurations, and the --no-* switches leave parts of a --full run out."""
import sys

import pytest

import bench


def parse(monkeypatch, *args):
    monkeypatch.setattr(sys, "argv", ["bench.py", *args])
    return bench.parse()


def test_plain_run_skips_everything_after_the_timed_region(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert not a.full and a.is_default and (a.steps, a.warmup, a.batch, a.model) == (7, 3, 256, "hil_speech")
    assert a.no_cpu_baseline and a.no_clock_probe and a.no_other_configs
    assert not a.no_launch_timing                       # launch timing is part of the timed steps


def test_full_run_keeps_the_extras(monkeypatch):
    a = parse(monkeypatch, "--full", "--steps", "7", "--warmup", "3")
    assert a.full and a.is_default and not (a.no_cpu_baseline or a.no_clock_probe or a.no_other_configs)
    a = parse(monkeypatch, "--full", "--no-clock-probe", "--batch", "8", "--other-configs")
    assert a.no_clock_probe and not a.no_cpu_baseline and a.other_configs and not a.is_default


def test_other_configs_needs_full(monkeypatch):
    with pytest.raises(SystemExit):
        parse(monkeypatch, "--batch", "8", "--other-configs")
