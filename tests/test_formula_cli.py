"""The `cudabrot` binary's --formula flag without a GPU: messages, refusals and exit codes follow the conventions of the
other extension flags (tests/test_power_cli.py): message, usage, exit 0; nothing is rendered.  What the flag means is
read from the `"projection"` and `"formula"` lines that --stats prints before any device is touched."""

import pytest

from cli_harness import IDENTITY, RUN_FLAGS, SMALL, both_orders, refused, run, stated
from cli_harness import exe  # noqa: F401 (a fixture)

NAMES = ["tricorn", "celtic", "buffalo", "perpendicular", "celtic-tricorn"]


BAD = "Invalid formula (want tricorn, celtic, buffalo, perpendicular or celtic-tricorn): "
FORMULA = ["--formula", "tricorn"]
OTHERS = (
    (["--power", "3"], "--formula does not combine with --power."),
    (["--burning-ship"], "--formula does not combine with --burning-ship."),
    (["--anti"], "--formula does not combine with --anti."),
    (["--focus"], "--formula does not combine with --focus."),
    (["--focus-level", "6"], "--formula does not combine with --focus."),
    (["--focus-probe", "8"], "--formula does not combine with --focus."),
    (["--focus-dilate", "2"], "--formula does not combine with --focus."),
    (["--channel", "9:1:x"], "--formula does not combine with --channel."),
    (["--color", "c.ppm"], "--formula does not combine with --channel."),
    (["--gpus", "2"], "--formula does not combine with --gpus above 1."),
)
REFUSED = both_orders(FORMULA, OTHERS)
# the flag's own refusal comes before those of --palette, --power, --julia and the projection, which the same command
# line would trip as well
PALETTE = ["--palette", "0:ffffff", "-m", "50"]
BEFORE_OTHERS = [(extra + FORMULA + o, line)
                 for extra in (["--plane", "zr,cr"], ["--julia", "0.3,0"], PALETTE, ["--julia", "0.3,0"] + PALETTE)
                 for o, line in OTHERS]
WITH_STATS = [(FORMULA + ["--stats"] + o, line) for o, line in OTHERS]


@pytest.mark.parametrize(
    "args,first_line",
    [
        (["--formula"], "Argument --formula needs a value."),
        (["--formula", ""], BAD),
        (["--formula", "mandelbrot"], BAD + "mandelbrot"),
        (["--formula", "Tricorn"], BAD + "Tricorn"),
        (["--formula", "tricorn "], BAD + "tricorn "),
        (["--formula", "celtic_tricorn"], BAD + "celtic_tricorn"),
        (["--formula", "mandelbar"], BAD + "mandelbar"),
        (["--formula", "1"], BAD + "1"),
        (["--formula", "0"], BAD + "0"),
        (["--formula", "celtic", "--formula", "ship"], BAD + "ship"),
    ]
    + REFUSED
    + BEFORE_OTHERS
    + WITH_STATS,
)
def test_formula_flag_prints_message_then_usage_and_exits_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


def test_usage_does_not_list_the_flag(exe):
    assert "--formula" not in run(exe, "--help").stdout


@pytest.mark.parametrize("name", NAMES)
def test_each_name_alone_is_the_identity_projection(exe, tmp_path, name):
    matrix, said = stated(exe, tmp_path, "--formula", name)
    assert matrix == IDENTITY
    assert said == {"formula": name}


@pytest.mark.parametrize("order", ["before", "after"])
def test_formula_takes_the_plane_that_is_given(exe, tmp_path, order):
    plane = ["--plane", "zr,cr", "--rotate", "zr,cr:90"]
    args = ["--formula", "buffalo"] + plane if order == "before" else plane + ["--formula", "buffalo"]
    matrix, said = stated(exe, tmp_path, *args)
    assert matrix == [0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0]
    assert said == {"formula": "buffalo"}
    matrix, said = stated(exe, tmp_path, "--project", "0.5,0,0,1:0,2,0,0", "--formula", "celtic-tricorn")
    assert matrix == [0.5, 0.0, 0.0, 1.0, 0.0, 2.0, 0.0, 0.0] and said == {"formula": "celtic-tricorn"}


def test_formula_combines_with_julia_palette_and_the_run_flags(exe, tmp_path):
    matrix, said = stated(exe, tmp_path, "--formula", "perpendicular", "--julia", "-0.8,0.156", "--palette",
                          "0:000030,49:ffffff", *RUN_FLAGS)
    assert matrix == IDENTITY
    assert [float.fromhex(v) for v in said.pop("julia")] == [-0.8, 0.156]
    assert said == {"formula": "perpendicular", "palette": [[0, "000030"], [49, "ffffff"]]}


def test_the_last_formula_counts(exe, tmp_path):
    assert stated(exe, tmp_path, "--formula", "tricorn", "--formula", "celtic")[1] == {"formula": "celtic"}


def test_without_the_flag_no_formula_line(exe, tmp_path):
    r = run(exe, *SMALL, "--plane", "zr,cr", cwd=tmp_path)
    assert "formula" not in r.stderr and "projection" in r.stderr.split("\n")[0]
