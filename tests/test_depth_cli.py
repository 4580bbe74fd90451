"""The `cudabrot` binary's --depth flag without a GPU: messages, refusals and exit codes follow the conventions of the
other extension flags (tests/test_formula_cli.py): message, usage, exit 0; nothing is rendered.  What the flag means is
read from the `"projection"` and `"depth"` lines that --stats prints before any device is touched."""

import pytest

from cli_harness import CHANNELS, IDENTITY, RUN_FLAGS, SMALL, both_orders, refused, run, stated
from cli_harness import exe  # noqa: F401 (a fixture)

BAD = ("Invalid depth (want ROW:MIN:MAX[:N], ROW an axis zr, zi, cr, ci or four numbers, MIN < MAX, N from 1 to 256): ")
DEPTH = ["--depth", "cr:-2:0.5:64"]
OTHERS = (
    (["--palette", "0:ffffff"], "--depth does not combine with --palette."),
    (["--anti"], "--depth does not combine with --anti."),
    (["--focus"], "--depth does not combine with --focus."),
    (["--focus-level", "6"], "--depth does not combine with --focus."),
    (["--focus-probe", "8"], "--depth does not combine with --focus."),
    (["--focus-dilate", "2"], "--depth does not combine with --focus."),
    (["--channel", "9:1:x"], "--depth does not combine with --channel."),
    (CHANNELS + ["--color", "c.ppm"], "--depth does not combine with --channel."),
    (["--gpus", "2"], "--depth does not combine with --gpus above 1."),
    (["--state-format", "raw"], "--depth does not combine with --state-format raw."),
)
REFUSED = both_orders(DEPTH, OTHERS)
# The flag's row is the table's last: where another flag's row applies to the same command line, that row has spoken
# already, with its own subject.  Recorded from the table, in both orders.
EARLIER_ROWS = (
    (["--palette", "0:ffffff", "--anti"], "--palette does not combine with --anti."),
    (["--palette", "0:ffffff", "--state-format", "raw"], "--palette does not combine with --state-format raw."),
    (["--palette", "0:ffffff", "-m", "0"], "--palette needs -m from 1 to 16777216."),
    (["--formula", "tricorn", "--anti"], "--formula does not combine with --anti."),
    (["--power", "3", "--focus"], "--power does not combine with --focus."),
    (["--julia", "0.3,0", "--gpus", "2"], "--julia does not combine with --gpus above 1."),
    (["--plane", "zr,cr", "--anti"], "A projection does not combine with --anti."),
    (["--rotate", "zr,cr:30", "--channel", "9:1:x"], "A projection does not combine with --channel."),
    (["--project", "1,0,0,0:0,1,0,0", "--plane", "zr,cr"], "--project does not combine with --plane or --rotate."),
    (["--focus", "--anti"], "--focus does not combine with --anti."),
    (["--anti", "--channel", "9:1:x"], "--anti does not combine with --channel."),
    (["--color", "c.ppm"], "--color needs exactly 3 --channel images, got 0."),
)
BEHIND = both_orders(DEPTH, EARLIER_ROWS)
WITH_STATS = [(DEPTH + ["--stats"] + o, line) for o, line in OTHERS]
MALFORMED = ["", "cr", "cr:", "cr:-2", "cr:-2:", "cr:-2:0.5:", "cr:-2:0.5:0", "cr:-2:0.5:257", "cr:-2:0.5:-1", "cr:-2:0.5:+4",
             "cr:-2:0.5:4.0", "cr:-2:0.5:4:", "cr:-2:0.5:4:1", "cr:1:1", "cr:1:0", "cr:nan:1", "cr:0:inf", "cr:-inf:0",
             "cr: -2:0.5", "cr:-2: 0.5", "cr:-2:0.5 ", " cr:-2:0.5", "xx:-2:0.5", "CR:-2:0.5", "zr,zi:-2:0.5", "cr,-2:0.5",
             "1,0,0:-2:0.5", "1,0,0,0,0:-2:0.5", "1,0,0,nan:-2:0.5", "1,0,0,inf:-2:0.5", "1,0,,0:-2:0.5", "1,0,0,0:-2",
             "1, 0,0,0:-2:0.5", "1:0:0:0:-2:0.5", "cr;-2;0.5", "cr:-2:0.5:0x10", "cr:a:b", "cr:-2:0.5:99999999999999999999"]


@pytest.mark.parametrize(
    "args,first_line",
    [(["--depth"], "Argument --depth needs a value.")]
    + [(["--depth", v], BAD + v) for v in MALFORMED]
    + [(["--plane", "zr,zi", "--depth", v, "-w", "16"], BAD + v) for v in MALFORMED[:6]]
    + [(["--depth", "cr:-2:0.5", "--depth", "cr:1:1"], BAD + "cr:1:1")]
    + REFUSED
    + BEHIND
    + WITH_STATS,
)
def test_depth_flag_prints_message_then_usage_and_exits_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


def test_usage_does_not_list_the_flag(exe):
    """The usage text is the reference's and lists no extension flag; README.md and DESIGN.md 4.16 describe this one."""
    assert "--depth" not in run(exe, "--help").stdout


def depth_of(said):
    d = said["depth"]
    assert sorted(d) == ["max", "min", "row", "slices"] and all(isinstance(v, str) for v in d["row"] + [d["min"], d["max"]])
    return [float.fromhex(v) for v in d["row"]], float.fromhex(d["min"]), float.fromhex(d["max"]), d["slices"]


@pytest.mark.parametrize("axis", ["zr", "zi", "cr", "ci"])
def test_an_axis_alone_is_the_identity_plane_and_a_unit_row(exe, tmp_path, axis):
    matrix, said = stated(exe, tmp_path, "--depth", axis + ":-0.02:0.02")
    assert matrix == IDENTITY
    row = [1.0 if a == axis else 0.0 for a in ("zr", "zi", "cr", "ci")]
    assert list(said) == ["depth"] and depth_of(said) == (row, -0.02, 0.02, 1)  # N defaults to 1


def test_accepted_forms(exe, tmp_path):
    assert depth_of(stated(exe, tmp_path, "--depth", "cr:-2:0.5:64")[1]) == ([0.0, 0.0, 1.0, 0.0], -2.0, 0.5, 64)
    assert depth_of(stated(exe, tmp_path, "--depth", "cr:-2:0.5:256")[1])[3] == 256
    assert depth_of(stated(exe, tmp_path, "--depth", "cr:-2:0.5:1")[1])[3] == 1
    assert depth_of(stated(exe, tmp_path, "--depth", "0.5,-0.25,1e-3,7:-1e9:+1e9:3")[1]) == (
        [0.5, -0.25, 1e-3, 7.0], -1e9, 1e9, 3)
    # hexfloats are taken, in the row and in the window
    assert depth_of(stated(exe, tmp_path, "--depth", "0x1p-1,0,-0x1.8p+0,0:-0x1p+1:0x1.999999999999ap-4:007")[1]) == (
        [0.5, 0.0, -1.5, 0.0], -2.0, 0.1, 7)
    # the last one counts
    assert depth_of(stated(exe, tmp_path, "--depth", "cr:-2:0.5:64", "--depth", "zi:0:1")[1]) == ([0.0, 1.0, 0.0, 0.0], 0.0, 1.0, 1)


@pytest.mark.parametrize("order", ["before", "after"])
def test_depth_takes_the_plane_that_is_given_and_rotate_does_not_turn_the_row(exe, tmp_path, order):
    plane = ["--plane", "zr,cr", "--rotate", "zr,cr:90"]
    flag = ["--depth", "zr:-2:2:4"]
    matrix, said = stated(exe, tmp_path, *(flag + plane if order == "before" else plane + flag))
    assert matrix == [0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0]
    assert depth_of(said) == ([1.0, 0.0, 0.0, 0.0], -2.0, 2.0, 4)  # the row is what the flag says
    matrix, said = stated(exe, tmp_path, "--project", "0.5,0,0,1:0,2,0,0", *flag)
    assert matrix == [0.5, 0.0, 0.0, 1.0, 0.0, 2.0, 0.0, 0.0] and depth_of(said)[3] == 4


def test_depth_combines_with_the_steps_julia_and_the_run_flags(exe, tmp_path):
    matrix, said = stated(exe, tmp_path, "--depth", "ci:-1:1:8", "--julia", "-0.8,0.156", "--power", "3", *RUN_FLAGS)
    assert matrix == IDENTITY
    assert [float.fromhex(v) for v in said.pop("julia")] == [-0.8, 0.156] and said.pop("power") == 3
    assert depth_of(said) == ([0.0, 0.0, 0.0, 1.0], -1.0, 1.0, 8)
    _, said = stated(exe, tmp_path, "--formula", "buffalo", "--depth", "ci:-1:1:8", "--tonemap", "thresholds")
    assert said.pop("formula") == "buffalo" and depth_of(said)[3] == 8
    _, said = stated(exe, tmp_path, "--burning-ship", "--depth", "ci:-1:1:8", "--state-format", "native")
    assert list(said) == ["depth"]


def test_without_the_flag_no_depth_line(exe, tmp_path):
    r = run(exe, *SMALL, "--plane", "zr,cr", cwd=tmp_path)
    assert "depth" not in r.stderr and "projection" in r.stderr.split("\n")[0]
