"""The `cudabrot` binary's --power flag without a GPU: messages, refusals and exit codes follow the conventions of the
other extension flags (tests/test_project_cli.py): message, usage, exit 0; nothing is rendered.  What the flag means is
read from the `"projection"` and `"power"` lines that --stats prints before any device is touched."""

import pytest

from cli_harness import IDENTITY, SMALL, both_orders, refused, run, stated
from cli_harness import exe  # noqa: F401 (a fixture)

BAD_POWER = "Invalid power (want an integer from 3 to 8): "
POWER = ["--power", "3"]
OTHERS = (
    (["--burning-ship"], "--power does not combine with --burning-ship."),
    (["--anti"], "--power does not combine with --anti."),
    (["--focus"], "--power does not combine with --focus."),
    (["--focus-level", "6"], "--power does not combine with --focus."),
    (["--focus-probe", "8"], "--power does not combine with --focus."),
    (["--focus-dilate", "2"], "--power does not combine with --focus."),
    (["--channel", "9:1:x"], "--power does not combine with --channel."),
    (["--color", "c.ppm"], "--power does not combine with --channel."),
    (["--gpus", "2"], "--power does not combine with --gpus above 1."),
)
REFUSED = both_orders(POWER, OTHERS)
# the flag's own refusal comes before the projection's, which the same command line would trip as well
WITH_PLANE = [(["--plane", "zr,cr"] + POWER + o, line) for o, line in OTHERS[1:]]
WITH_STATS = [(POWER + ["--stats"] + o, line) for o, line in OTHERS] + [(o + ["--stats"] + POWER, line) for o, line in OTHERS]


@pytest.mark.parametrize(
    "args,first_line",
    [
        (["--power"], "Argument --power needs a value."),
        (["--power", ""], BAD_POWER),
        (["--power", "2"], BAD_POWER + "2"),
        (["--power", "9"], BAD_POWER + "9"),
        (["--power", "0"], BAD_POWER + "0"),
        (["--power", "1"], BAD_POWER + "1"),
        (["--power", "-3"], BAD_POWER + "-3"),
        (["--power", "3.0"], BAD_POWER + "3.0"),
        (["--power", "2.5"], BAD_POWER + "2.5"),
        (["--power", "3x"], BAD_POWER + "3x"),
        (["--power", "three"], BAD_POWER + "three"),
        (["--power", "3 "], BAD_POWER + "3 "),
        (["--power", "99999999999999999999"], BAD_POWER + "99999999999999999999"),
        (["--power", "4", "--power", "12"], BAD_POWER + "12"),
    ]
    + REFUSED
    + WITH_PLANE
    + WITH_STATS,
)
def test_power_flag_prints_message_then_usage_and_exits_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


def test_usage_does_not_list_the_flag(exe):
    assert "--power" not in run(exe, "--help").stdout


@pytest.mark.parametrize("degree", range(3, 9))
def test_power_alone_is_the_identity_projection(exe, tmp_path, degree):
    matrix, said = stated(exe, tmp_path, "--power", str(degree))
    assert matrix == IDENTITY
    assert said == {"power": degree}


@pytest.mark.parametrize("order", ["before", "after"])
def test_power_takes_the_plane_that_is_given(exe, tmp_path, order):
    plane = ["--plane", "zr,cr", "--rotate", "zr,cr:90"]
    args = ["--power", "5"] + plane if order == "before" else plane + ["--power", "5"]
    matrix, said = stated(exe, tmp_path, *args)
    assert matrix == [0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0]
    assert said == {"power": 5}
    matrix, said = stated(exe, tmp_path, "--project", "0.5,0,0,1:0,2,0,0", "--power", "8")
    assert matrix == [0.5, 0.0, 0.0, 1.0, 0.0, 2.0, 0.0, 0.0] and said == {"power": 8}


def test_the_last_power_counts(exe, tmp_path):
    assert stated(exe, tmp_path, "--power", "3", "--power", "7")[1] == {"power": 7}


def test_without_the_flag_no_power_line(exe, tmp_path):
    r = run(exe, *SMALL, "--plane", "zr,cr", cwd=tmp_path)
    assert "power" not in r.stderr and "projection" in r.stderr.split("\n")[0]
