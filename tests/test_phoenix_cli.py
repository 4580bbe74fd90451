"""The `cudabrot` binary's --phoenix flag without a GPU: messages, refusals and exit codes follow the conventions of the
other extension flags (tests/test_frames_cli.py): message, usage, exit 0; nothing is rendered.  What the flag means is read
from the `"projection"`, `"julia"` and `"phoenix"` lines that --stats prints before any device is touched."""

import pytest

from cli_harness import CHANNELS, IDENTITY, RUN_FLAGS, SMALL, both_orders, refused, run, stated
from cli_harness import exe  # noqa: F401 (a fixture)

BAD = "Invalid phoenix parameter (want RE,IM, two numbers from -2 to 2): "
PHOENIX = ["--phoenix", "-0.5,0"]
# the row's partners, in its order
OTHERS = (
    (["--power", "3"], "--phoenix does not combine with --power."),
    (["--formula", "tricorn"], "--phoenix does not combine with --formula."),
    (["--burning-ship"], "--phoenix does not combine with --burning-ship."),
    (["--palette", "0:ffffff"], "--phoenix does not combine with --palette."),
    (["--depth", "cr:-2:0.5:4"], "--phoenix does not combine with --depth."),
    (["--depth", "cr:-2:0.5:4", "--depth-palette", "0:ffffff"], "--phoenix does not combine with --depth."),
    (["--sweep", "zi,cr:0:90:4"], "--phoenix does not combine with --sweep."),
    (["--anti"], "--phoenix does not combine with --anti."),
    (["--focus"], "--phoenix does not combine with --focus."),
    (["--focus-level", "6"], "--phoenix does not combine with --focus."),
    (["--channel", "9:1:x"], "--phoenix does not combine with --channel."),
    (CHANNELS + ["--color", "c.ppm"], "--phoenix does not combine with --channel."),
    (["--gpus", "2"], "--phoenix does not combine with --gpus above 1."),
    # the first partner present speaks
    (["--power", "3", "--palette", "0:ffffff"], "--phoenix does not combine with --power."),
    (["--burning-ship", "--depth", "cr:-2:0.5:4"], "--phoenix does not combine with --burning-ship."),
    (["--julia", "0.3,0", "--sweep", "zi,cr:0:90:4"], "--phoenix does not combine with --sweep."),
)
REFUSED = both_orders(PHOENIX, OTHERS)
# The flag's row is the table's last: where an older row applies to the same command line, that row has spoken already,
# with its own subject.  In both orders.
EARLIER_ROWS = (
    (["--power", "3", "--focus"], "--power does not combine with --focus."),
    (["--palette", "0:ffffff", "--anti"], "--palette does not combine with --anti."),
    (["--formula", "tricorn", "--anti"], "--formula does not combine with --anti."),
    (["--formula", "tricorn", "--power", "3"], "--formula does not combine with --power."),
    (["--julia", "0.3,0", "--gpus", "2"], "--julia does not combine with --gpus above 1."),
    (["--plane", "zr,cr", "--anti"], "A projection does not combine with --anti."),
    (["--rotate", "zr,cr:30", "--channel", "9:1:x"], "A projection does not combine with --channel."),
    (["--project", "1,0,0,0:0,1,0,0", "--plane", "zr,cr"], "--project does not combine with --plane or --rotate."),
    (["--focus", "--anti"], "--focus does not combine with --anti."),
    (["--anti", "--channel", "9:1:x"], "--anti does not combine with --channel."),
    (["--color", "c.ppm"], "--color needs exactly 3 --channel images, got 0."),
    (["--depth", "cr:-2:0.5:4", "--anti"], "--depth does not combine with --anti."),
    (["--depth-palette", "0:ffffff"], "--depth-palette needs --depth."),
    (["--sweep", "zi,cr:0:90:4", "--depth", "cr:-2:0.5:4"], "--sweep does not combine with --depth."),
    (["--palette", "0:ffffff", "--state-format", "raw"], "--palette does not combine with --state-format raw."),
)
BEHIND = both_orders(PHOENIX, EARLIER_ROWS)
WITH_STATS = [(PHOENIX + ["--stats"] + o, line) for o, line in OTHERS]
MALFORMED = ["", "0", "0,", ",0", "0,0,", "0,0,0", "0 ,0", "0, 0", " 0,0", "0,0 ", "0;0", "a,b", "nan,0", "0,nan", "inf,0",
             "0,-inf", "2.0000001,0", "0,-2.0000001", "0x1.0000000000001p+1,0", "3,0", "0:0", "1e400,0"]


@pytest.mark.parametrize(
    "args,first_line",
    [(["--phoenix"], "Argument --phoenix needs a value.")]
    + [(["--phoenix", v], BAD + v) for v in MALFORMED]
    + [(["--julia", "0.3,0", "--phoenix", v, "-w", "16"], BAD + v) for v in MALFORMED[:6]]
    # a repeated flag validates each value
    + [(["--phoenix", "9,9", "--phoenix", "0,0"], BAD + "9,9"), (["--phoenix", "0,0", "--phoenix", "9,9"], BAD + "9,9")]
    + REFUSED
    + BEHIND
    + WITH_STATS,
)
def test_phoenix_flag_prints_message_then_usage_and_exits_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


def test_usage_does_not_list_the_flag(exe):
    """The usage text is the reference's and lists no extension flag; README.md and DESIGN.md 4.19 describe this one."""
    assert "--phoenix" not in run(exe, "--help").stdout


def p_of(said):
    return [float.fromhex(v) for v in said["phoenix"]]


def test_the_flag_alone_is_the_identity_plane_with_a_sampled_c(exe, tmp_path):
    matrix, said = stated(exe, tmp_path, "--phoenix", "-0.5,0")
    assert matrix == IDENTITY
    assert list(said) == ["phoenix"] and p_of(said) == [-0.5, 0.0]


def test_the_stats_line_is_two_hexfloats(exe, tmp_path):
    r = run(exe, *SMALL, "--phoenix", "0.3,-0.4", cwd=tmp_path)
    assert r.stderr.split("\n")[1] == '{"phoenix": ["%s", "%s"]}' % ("0x1.3333333333333p-2", "-0x1.999999999999ap-2")


def test_accepted_forms(exe, tmp_path):
    assert p_of(stated(exe, tmp_path, "--phoenix", "0x1p-1,-0x1.8p+0")[1]) == [0.5, -1.5]  # hexfloats
    assert p_of(stated(exe, tmp_path, "--phoenix", "2,-2")[1]) == [2.0, -2.0]  # the bounds are allowed
    assert p_of(stated(exe, tmp_path, "--phoenix", "+1e-1,.25")[1]) == [0.1, 0.25]
    assert p_of(stated(exe, tmp_path, "--phoenix", "0,0")[1]) == [0.0, 0.0]  # p = 0 is allowed
    assert p_of(stated(exe, tmp_path, "--phoenix", "1,1", "--phoenix", "0.25,0")[1]) == [0.25, 0.0]  # the last value


@pytest.mark.parametrize("first", ["julia", "phoenix"])
def test_it_combines_with_julia_a_plane_and_the_run_flags(exe, tmp_path, first):
    julia, flag = ["--julia", "0.56667,0"], ["--phoenix", "-0.5,0"]
    args = (julia + flag if first == "julia" else flag + julia) + ["--plane", "zr,cr"] + RUN_FLAGS + ["--state-format", "raw"]
    matrix, said = stated(exe, tmp_path, *args)
    assert matrix == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert list(said) == ["julia", "phoenix"]
    assert [float.fromhex(v) for v in said["julia"]] == [0.56667, 0.0] and p_of(said) == [-0.5, 0.0]
    matrix, said = stated(exe, tmp_path, "--rotate", "zr,cr:90", *flag, "--tonemap", "thresholds")
    assert matrix == [0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0] and list(said) == ["phoenix"]
    matrix, said = stated(exe, tmp_path, *flag, "--project", "0.5,0,0,1:0,2,0,0")
    assert matrix == [0.5, 0.0, 0.0, 1.0, 0.0, 2.0, 0.0, 0.0] and list(said) == ["phoenix"]


def test_without_the_flag_no_phoenix_line(exe, tmp_path):
    r = run(exe, *SMALL, "--julia", "0.3,0", cwd=tmp_path)
    assert "phoenix" not in r.stderr and "projection" in r.stderr.split("\n")[0]
