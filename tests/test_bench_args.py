"""bench.py's command line: a plain run times the headline alone, --full brings back the checks, baselines and extra lines,
--steps sets the timed steps, --dump-outputs is taken for the mxv workloads only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_headline_alone(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_cpu_baseline and a.no_extra and a.no_warm_build


def test_full_keeps_todays_run(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not (a.no_cpu_baseline or a.no_extra or a.no_warm_build)
    a = _parse(monkeypatch, "--full", "--no-extra")
    assert a.no_extra and not a.no_cpu_baseline


def test_dump_outputs_and_steps_arguments(monkeypatch, tmp_path):
    assert _parse(monkeypatch, "--dump-outputs", str(tmp_path)).dump_outputs == str(tmp_path)
    assert _parse(monkeypatch, "--workload", "kron26", "--dump-outputs", str(tmp_path)).dump_outputs == str(tmp_path)
    for argv in (["--workload", "mxm_plus_times", "--dump-outputs", str(tmp_path)], ["--steps", "0"]):
        with pytest.raises(SystemExit):
            _parse(monkeypatch, *argv)
