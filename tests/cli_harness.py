"""What the flag suites of the `cudabrot` binary share (tests/test_*_cli.py) -- test infrastructure only: the binary as a
fixture, the check of a refused command line, what an accepted one states under --stats before any device is touched, and
the constants the case tables are written with.  A fixture imported into a test module is a fixture of that module; `run`
is tools/gpu_launches.py's, which tests/device_launches.py hands on under its own name, re-exported here, and plot_harness
re-exports `exe` and `run` for the GPU suites."""

import json
import os

import pytest

from device_launches import run  # noqa: F401 (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
CHANNELS = ["--channel", "9:1:a", "--channel", "9:2:b", "--channel", "9:3:c"]
# the flags of a run that every plotted render takes beside its own
RUN_FLAGS = ["-m", "50", "-c", "5", "--seed", "7", "--kernel", "simple", "--tonemap", "host", "-g", "2.2", "-s", "buffer.bin",
             "--rng-state", "side.rng"]
SMALL = ["--stats", "--passes", "0", "-w", "16", "-h", "16"]  # what stated() runs a command line with


@pytest.fixture(scope="module")
def exe():
    path = os.path.join(ROOT, "cudabrot")
    if not os.access(path, os.X_OK):
        pytest.fail("./cudabrot is not built (run `make` or __graft_entry__.build())")
    return path


def both_orders(flag_words, rows):
    """The cases of `rows`, (other words, first line), with the flag's words in front of the others, then behind them."""
    return [(flag_words + o, line) for o, line in rows] + [(o + flag_words, line) for o, line in rows]


def refused(exe, args, first_line, tmp_path):
    """A command line the parser refuses: its message, the usage text, exit 0; nothing on stderr and nothing written."""
    r = run(exe, *args, cwd=tmp_path)
    assert r.returncode == 0
    lines = r.stdout.split("\n")
    assert lines[0] == first_line
    assert lines[1] == "Usage: %s [options]" % exe
    assert r.stdout.rstrip().endswith("include in the output image. Defaults to 2.0.")  # the usage text is the reference's
    assert r.stderr == ""  # decided before anything is printed under --stats and before any device is touched
    assert os.listdir(tmp_path) == []


def stats_lines(exe, tmp_path, *args):
    """The lines of stderr of an accepted command line on a 16 x 16 canvas under --stats.  The run itself goes on to the
    device (and ends there on a box without one); its outcome is not looked at."""
    r = run(exe, *SMALL, *args, cwd=tmp_path)
    assert "Usage:" not in r.stdout  # accepted: on to the device
    assert r.stdout.startswith("Creating 16x16 image")
    return r.stderr.split("\n")


def stated(exe, tmp_path, *args):
    """What a command line means, as the binary states it on stderr under --stats: the matrix on the first line, then one
    JSON object of one key per line, up to the first line that is none -> (matrix, {key: value} in the order stated).  The
    period palette's line is the one that carries a second key, its "period_eps"; both are taken.  What the run prints
    after the lines that state it -- the counters' line, where there is a device -- is dropped."""
    lines = stats_lines(exe, tmp_path, *args)
    values = json.loads(lines[0])["projection"]
    assert len(values) == 8
    said = {}
    for line in lines[1:]:
        try:
            obj = json.loads(line)
        except ValueError:
            break
        if not isinstance(obj, dict) or len(obj) != 1 and list(obj) != ["period_palette", "period_eps"]:
            break
        said.update(obj)
    return [float.fromhex(v) for v in values], said
