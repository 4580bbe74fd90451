"""The `cudabrot` binary's --julia flag without a GPU: messages, refusals and exit codes follow the conventions of the
other extension flags (tests/test_power_cli.py): message, usage, exit 0; nothing is rendered.  What the flag means is
read from the `"projection"`, `"power"` and `"julia"` lines that --stats prints before any device is touched."""

import pytest

from cli_harness import IDENTITY, SMALL, both_orders, refused, run, stated
from cli_harness import exe  # noqa: F401 (a fixture)

BAD_JULIA = "Invalid julia parameter (want RE,IM, two numbers from -2 to 2): "
JULIA = ["--julia", "-0.8,0.156"]
OTHERS = (
    (["--anti"], "--julia does not combine with --anti."),
    (["--focus"], "--julia does not combine with --focus."),
    (["--focus-level", "6"], "--julia does not combine with --focus."),
    (["--focus-probe", "8"], "--julia does not combine with --focus."),
    (["--focus-dilate", "2"], "--julia does not combine with --focus."),
    (["--channel", "9:1:x"], "--julia does not combine with --channel."),
    (["--color", "c.ppm"], "--julia does not combine with --channel."),
    (["--gpus", "2"], "--julia does not combine with --gpus above 1."),
)
REFUSED = both_orders(JULIA, OTHERS)
WITH_STATS = [(JULIA + ["--stats"] + o, line) for o, line in OTHERS] + [(o + ["--stats"] + JULIA, line) for o, line in OTHERS]
# the flag's own refusal comes before the projection's, which the same command line would trip as well
WITH_PLANE = [(["--plane", "zr,zi"] + JULIA + o, line) for o, line in OTHERS] + [
    (o + JULIA + ["--plane", "zr,zi"], line) for o, line in OTHERS]
# ... and after the Multibrot step's
AFTER_POWER = [
    (JULIA + ["--power", "3", "--burning-ship"], "--power does not combine with --burning-ship."),
    (["--power", "3"] + JULIA + ["--anti"], "--power does not combine with --anti."),
    (JULIA + ["--gpus", "2", "--power", "3"], "--power does not combine with --gpus above 1."),
]


@pytest.mark.parametrize(
    "args,first_line",
    [
        (["--julia"], "Argument --julia needs a value."),
        (["--julia", ""], BAD_JULIA),
        (["--julia", "0.5"], BAD_JULIA + "0.5"),
        (["--julia", "0.5,"], BAD_JULIA + "0.5,"),
        (["--julia", ",0.5"], BAD_JULIA + ",0.5"),
        (["--julia", "0.1,0.2,0.3"], BAD_JULIA + "0.1,0.2,0.3"),
        (["--julia", "nan,0"], BAD_JULIA + "nan,0"),
        (["--julia", "0,nan"], BAD_JULIA + "0,nan"),
        (["--julia", "inf,0"], BAD_JULIA + "inf,0"),
        (["--julia", "0,-inf"], BAD_JULIA + "0,-inf"),
        (["--julia", "2.5,0"], BAD_JULIA + "2.5,0"),
        (["--julia", "0,-2.0000001"], BAD_JULIA + "0,-2.0000001"),
        (["--julia", "0.1,0.2x"], BAD_JULIA + "0.1,0.2x"),
        (["--julia", "0.1x,0.2"], BAD_JULIA + "0.1x,0.2"),
        (["--julia", "0.1, 0.2"], BAD_JULIA + "0.1, 0.2"),
        (["--julia", " 0.1,0.2"], BAD_JULIA + " 0.1,0.2"),
        (["--julia", "0.1,0.2 "], BAD_JULIA + "0.1,0.2 "),
        (["--julia", "0.1:0.2"], BAD_JULIA + "0.1:0.2"),
        (["--julia", "0,0", "--julia", "3,0"], BAD_JULIA + "3,0"),
    ]
    + REFUSED
    + WITH_STATS
    + WITH_PLANE
    + AFTER_POWER,
)
def test_julia_flag_prints_message_then_usage_and_exits_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


def test_usage_does_not_list_the_flag(exe):
    assert "--julia" not in run(exe, "--help").stdout


def with_c(said):
    """What was stated, the "%a" texts of c as the doubles."""
    return dict(said, julia=[float.fromhex(v) for v in said["julia"]])


def test_julia_alone_is_the_identity_projection(exe, tmp_path):
    matrix, said = stated(exe, tmp_path, "--julia", "-0.8,0.156")
    assert matrix == IDENTITY
    assert with_c(said) == {"julia": [-0.8, 0.156]}


@pytest.mark.parametrize("text,c", [("-2,2", (-2.0, 2.0)), ("0x1.8p-1,-0x1p-3", (0.75, -0.125)), ("0,-0", (0.0, -0.0)),
                                    ("1e-3,+2.0", (0.001, 2.0))])
def test_julia_values_are_read_as_strtod_reads_them(exe, tmp_path, text, c):
    _, said = stated(exe, tmp_path, "--julia", text)
    assert [v.hex() for v in with_c(said)["julia"]] == [c[0].hex(), c[1].hex()]  # (the sign of a zero included)


@pytest.mark.parametrize("order", ["before", "after"])
def test_julia_takes_the_plane_and_the_step_that_are_given(exe, tmp_path, order):
    plane = ["--plane", "zr,cr", "--rotate", "zr,cr:90", "--power", "5"]
    args = JULIA + plane if order == "before" else plane + JULIA
    matrix, said = stated(exe, tmp_path, *args)
    assert matrix == [0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0]
    assert with_c(said) == {"power": 5, "julia": [-0.8, 0.156]}
    matrix, said = stated(exe, tmp_path, "--project", "0.5,0,0,1:0,2,0,0", "--burning-ship", *JULIA)
    assert matrix == [0.5, 0.0, 0.0, 1.0, 0.0, 2.0, 0.0, 0.0] and list(said) == ["julia"]


def test_the_last_julia_counts(exe, tmp_path):
    assert with_c(stated(exe, tmp_path, "--julia", "1,1", "--julia", "0.5,-0.25")[1]) == {"julia": [0.5, -0.25]}


def test_without_the_flag_no_julia_line(exe, tmp_path):
    r = run(exe, *SMALL, "--power", "3", cwd=tmp_path)
    assert "julia" not in r.stderr and "projection" in r.stderr.split("\n")[0]
