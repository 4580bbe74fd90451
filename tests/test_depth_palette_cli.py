"""The `cudabrot` binary's --depth-palette flag without a GPU: messages, refusals and exit codes follow the conventions of
the other extension flags (tests/test_depth_cli.py): message, usage, exit 0; nothing is rendered.  What the flag means is
read from the `"depth"` and `"depth_palette"` lines that --stats prints before any device is touched."""

import pytest

from cli_harness import CHANNELS, IDENTITY, RUN_FLAGS, both_orders, refused, run, stated
from cli_harness import exe  # noqa: F401 (a fixture)

BAD = "Invalid depth palette (want K:RRGGBB,... K ascending, at most 16 stops): "
NEEDS = "--depth-palette needs --depth."
DEPTH = ["--depth", "cr:-2:0.5:64"]
COLOURS = ["--depth-palette", "0:000030,32:ff8000,63:ffffff"]
# What the binary before this flag answered to DEPTH + these (recorded from it, in both orders of the two): the answer
# with --depth-palette on the line as well is the same, because --depth's row of the refusal table, and every row before
# it, speaks before the flag's own.
WITH_DEPTH = (
    (["--palette", "0:ffffff"], "--depth does not combine with --palette."),
    (["--anti"], "--depth does not combine with --anti."),
    (["--focus"], "--depth does not combine with --focus."),
    (["--focus-level", "6"], "--depth does not combine with --focus."),
    (["--channel", "9:1:x"], "--depth does not combine with --channel."),
    (CHANNELS + ["--color", "c.ppm"], "--depth does not combine with --channel."),
    (["--gpus", "2"], "--depth does not combine with --gpus above 1."),
    (["--state-format", "raw"], "--depth does not combine with --state-format raw."),
    (["--palette", "0:ffffff", "--anti"], "--palette does not combine with --anti."),
    (["--palette", "0:ffffff", "-m", "0"], "--palette needs -m from 1 to 16777216."),
    (["--formula", "tricorn", "--anti"], "--formula does not combine with --anti."),
    (["--power", "3", "--focus"], "--power does not combine with --focus."),
    (["--julia", "0.3,0", "--gpus", "2"], "--julia does not combine with --gpus above 1."),
    (["--plane", "zr,cr", "--anti"], "A projection does not combine with --anti."),
    (["--color", "c.ppm"], "--color needs exactly 3 --channel images, got 0."),
)
UNCHANGED = ([(DEPTH + COLOURS + o, line) for o, line in WITH_DEPTH] + [(o + COLOURS + DEPTH, line) for o, line in WITH_DEPTH]
             + [(COLOURS + o + DEPTH + ["--stats"], line) for o, line in WITH_DEPTH])
# Without --depth, where the binary before this flag had an answer for the rest of the line, that answer stands; where it
# had none, the flag's own row -- the table's last -- speaks.
WITHOUT_DEPTH = (
    ([], NEEDS),
    (["--plane", "zr,cr"], NEEDS),
    (["--julia", "0.3,0", "--power", "3"], NEEDS),
    (["--palette", "0:ffffff"], NEEDS),
    (["--anti"], NEEDS),
    (["--gpus", "2"], NEEDS),
    (["--palette", "0:ffffff", "--anti"], "--palette does not combine with --anti."),
    (["--focus", "--anti"], "--focus does not combine with --anti."),
    (["--color", "c.ppm"], "--color needs exactly 3 --channel images, got 0."),
)
ALONE = both_orders(COLOURS, WITHOUT_DEPTH)
MALFORMED = ["", "0", "0:", "0:fff", "0:fffffff", "0:gggggg", "0:ffffff,", ",0:ffffff", "0:ffffff,0:000000", "5:ffffff,3:000000",
             "-1:ffffff", "+1:ffffff", "1.0:ffffff", " 0:ffffff", "0:ffffff ", "0: ffffff", "0;ffffff", "0:ffffff;1:000000",
             "0:#ffffff", "0:0xffff", "99999999999:ffffff", ",".join("%d:ffffff" % k for k in range(17))]


@pytest.mark.parametrize(
    "args,first_line",
    [(["--depth-palette"], "Argument --depth-palette needs a value.")]
    + [(["--depth-palette", v], BAD + v) for v in MALFORMED]
    + [(DEPTH + ["--depth-palette", v, "-w", "16"], BAD + v) for v in MALFORMED[:6]]
    + [(DEPTH + COLOURS + ["--depth-palette", "0:fff"], BAD + "0:fff")]
    + UNCHANGED
    + ALONE,
)
def test_depth_palette_flag_prints_message_then_usage_and_exits_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


def test_usage_is_unchanged_and_does_not_list_the_flag(exe):
    """The usage text is the reference's and lists no extension flag; README.md and DESIGN.md 4.17 describe this one."""
    out = run(exe, "--help").stdout
    assert "--depth-palette" not in out and "--depth" not in out
    assert out.rstrip().split("\n")[-1] == "             include in the output image. Defaults to 2.0."


def test_the_stops_are_stated_beside_the_depth(exe, tmp_path):
    matrix, said = stated(exe, tmp_path, "--depth", "cr:-2:0.5:256", "--depth-palette", "0:000030,128:Ff8000,255:ffffff")
    assert matrix == IDENTITY
    assert list(said) == ["depth", "depth_palette"]
    assert said["depth"]["slices"] == 256
    assert said["depth_palette"] == [[0, "000030"], [128, "ff8000"], [255, "ffffff"]]
    # either order of the two flags, one stop, and stops at or above N are taken as --palette takes stops at or above -m
    _, said = stated(exe, tmp_path, "--depth-palette", "7:010203", "--depth", "zi:-1:1:4")
    assert said["depth_palette"] == [[7, "010203"]] and said["depth"]["slices"] == 4
    _, said = stated(exe, tmp_path, "--depth", "zi:-1:1", "--depth-palette", "0:000000,1000:ffffff")
    assert said["depth_palette"] == [[0, "000000"], [1000, "ffffff"]] and said["depth"]["slices"] == 1
    # the last one counts
    _, said = stated(exe, tmp_path, *DEPTH, *COLOURS, "--depth-palette", "3:0a0b0c")
    assert said["depth_palette"] == [[3, "0a0b0c"]]


def test_it_combines_with_the_steps_julia_the_plane_and_the_run_flags(exe, tmp_path):
    matrix, said = stated(exe, tmp_path, *COLOURS, "--depth", "ci:-1:1:8", "--julia", "-0.8,0.156", "--power", "3",
                          "--plane", "zr,cr", *RUN_FLAGS)
    assert matrix == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert list(said) == ["power", "julia", "depth", "depth_palette"]
    _, said = stated(exe, tmp_path, "--formula", "buffalo", *DEPTH, *COLOURS, "--tonemap", "thresholds")
    assert list(said) == ["formula", "depth", "depth_palette"]
    _, said = stated(exe, tmp_path, "--burning-ship", *DEPTH, *COLOURS, "--state-format", "native")
    assert list(said) == ["depth", "depth_palette"]


def test_without_the_flag_no_depth_palette_line(exe, tmp_path):
    _, said = stated(exe, tmp_path, *DEPTH)
    assert list(said) == ["depth"]
