"""The `cudabrot` binary's --sweep flag without a GPU: messages, refusals and exit codes follow the conventions of the
other extension flags (tests/test_depth_cli.py): message, usage, exit 0; nothing is rendered.  What the flag means is read
from the `"projection"` and `"sweep"` lines that --stats prints before any device is touched."""

import pytest

from cli_harness import CHANNELS, IDENTITY, RUN_FLAGS, SMALL, both_orders, refused, run, stated
from cli_harness import exe  # noqa: F401 (a fixture)

BAD = ("Invalid sweep (want X,Y:DEG0:DEG1:F, two different axes of zr, zi, cr, ci, two finite angles and 1 to 256 frames): ")
SWEEP = ["--sweep", "zi,cr:0:90:64"]
OTHERS = (
    (["--palette", "0:ffffff"], "--sweep does not combine with --palette."),
    (["--depth", "cr:-2:0.5:4"], "--sweep does not combine with --depth."),
    (["--depth", "cr:-2:0.5:4", "--depth-palette", "0:ffffff"], "--sweep does not combine with --depth."),
    (["--anti"], "--sweep does not combine with --anti."),
    (["--focus"], "--sweep does not combine with --focus."),
    (["--focus-level", "6"], "--sweep does not combine with --focus."),
    (["--channel", "9:1:x"], "--sweep does not combine with --channel."),
    (CHANNELS + ["--color", "c.ppm"], "--sweep does not combine with --channel."),
    (["--gpus", "2"], "--sweep does not combine with --gpus above 1."),
    (["--state-format", "raw"], "--sweep does not combine with --state-format raw."),
)
REFUSED = both_orders(SWEEP, OTHERS)
# The flag's row is the table's last: where an older row applies to the same command line, that row has spoken already,
# with its own subject.  In both orders.
EARLIER_ROWS = (
    (["--palette", "0:ffffff", "--anti"], "--palette does not combine with --anti."),
    (["--formula", "tricorn", "--anti"], "--formula does not combine with --anti."),
    (["--power", "3", "--focus"], "--power does not combine with --focus."),
    (["--julia", "0.3,0", "--gpus", "2"], "--julia does not combine with --gpus above 1."),
    (["--plane", "zr,cr", "--anti"], "A projection does not combine with --anti."),
    (["--rotate", "zr,cr:30", "--channel", "9:1:x"], "A projection does not combine with --channel."),
    (["--project", "1,0,0,0:0,1,0,0", "--plane", "zr,cr"], "--project does not combine with --plane or --rotate."),
    (["--focus", "--anti"], "--focus does not combine with --anti."),
    (["--anti", "--channel", "9:1:x"], "--anti does not combine with --channel."),
    (["--color", "c.ppm"], "--color needs exactly 3 --channel images, got 0."),
    (["--depth", "cr:-2:0.5:4", "--anti"], "--depth does not combine with --anti."),
    (["--depth-palette", "0:ffffff"], "--depth-palette needs --depth."),
)
BEHIND = both_orders(SWEEP, EARLIER_ROWS)
WITH_STATS = [(SWEEP + ["--stats"] + o, line) for o, line in OTHERS]
MALFORMED = ["", "zi", "zi,cr", "zi,cr:", "zi,cr:0", "zi,cr:0:", "zi,cr:0:90", "zi,cr:0:90:", "zi,cr:0:90:0", "zi,cr:0:90:257",
             "zi,cr:0:90:-1", "zi,cr:0:90:+4", "zi,cr:0:90:4.0", "zi,cr:0:90:4:", "zi,cr:0:90:4:1", "zi,zi:0:90:4",
             "zi,xx:0:90:4", "ZI,CR:0:90:4", "zi:cr:0:90:4", "zi,cr,0,90,4", "zi,cr:nan:90:4", "zi,cr:0:inf:4",
             "zi,cr:-inf:0:4", "zi,cr: 0:90:4", "zi,cr:0: 90:4", "zi,cr:0:90:4 ", " zi,cr:0:90:4", "zi,cr:0:90:0x10",
             "zi,cr:a:b:4", "zi,cr:0:90:99999999999999999999", "1,2:0:90:4"]


@pytest.mark.parametrize(
    "args,first_line",
    [(["--sweep"], "Argument --sweep needs a value.")]
    + [(["--sweep", v], BAD + v) for v in MALFORMED]
    + [(["--plane", "zr,zi", "--sweep", v, "-w", "16"], BAD + v) for v in MALFORMED[:6]]
    + [(["--sweep", "zi,cr:0:90:4", "--sweep", "zi,cr:0:90:8"], BAD + "zi,cr:0:90:8")]  # at most once
    + REFUSED
    + BEHIND
    + WITH_STATS,
)
def test_sweep_flag_prints_message_then_usage_and_exits_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


def test_usage_does_not_list_the_flag(exe):
    """The usage text is the reference's and lists no extension flag; README.md and DESIGN.md 4.18 describe this one."""
    assert "--sweep" not in run(exe, "--help").stdout


def sweep_of(said):
    s = said["sweep"]
    assert sorted(s) == ["angles", "axes", "frames", "from", "to"] and len(s["angles"]) == s["frames"]
    return s["axes"], float.fromhex(s["from"]), float.fromhex(s["to"]), [float.fromhex(a) for a in s["angles"]]


def test_the_flag_alone_sweeps_the_identity_plane(exe, tmp_path):
    matrix, said = stated(exe, tmp_path, "--sweep", "zi,cr:0:90:4")
    assert matrix == IDENTITY  # the base: frame 0 of a sweep from 0
    assert list(said) == ["sweep"] and sweep_of(said) == (["zi", "cr"], 0.0, 90.0, [0.0, 22.5, 45.0, 67.5])


def test_accepted_forms(exe, tmp_path):
    assert sweep_of(stated(exe, tmp_path, "--sweep", "cr,zr:-10.5:+1e2:1")[1]) == (["cr", "zr"], -10.5, 100.0, [-10.5])
    axes, lo, hi, angles = sweep_of(stated(exe, tmp_path, "--sweep", "zr,ci:0x1p+2:0x1.8p+5:003")[1])  # hexfloats, 003
    assert (axes, lo, hi) == (["zr", "ci"], 4.0, 48.0) and angles == [4.0 + ((48.0 - 4.0) * f) / 3.0 for f in range(3)]
    assert len(sweep_of(stated(exe, tmp_path, "--sweep", "zi,cr:0:360:256")[1])[3]) == 256
    # deg1 is exclusive and may lie below deg0
    assert sweep_of(stated(exe, tmp_path, "--sweep", "zi,cr:90:0:2")[1])[3] == [90.0, 45.0]


@pytest.mark.parametrize("order", ["before", "after", "between"])
def test_the_sweep_is_applied_last_wherever_it_stands(exe, tmp_path, order):
    plane, rotate, flag = ["--plane", "zr,cr"], ["--rotate", "zr,cr:90"], ["--sweep", "zi,cr:0:90:2"]
    args = {"before": flag + plane + rotate, "after": plane + rotate + flag, "between": plane + flag + rotate}[order]
    matrix, said = stated(exe, tmp_path, *args)
    assert matrix == [0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0]  # the base is the plane after every --plane / --rotate
    assert sweep_of(said)[3] == [0.0, 45.0]
    matrix, said = stated(exe, tmp_path, "--project", "0.5,0,0,1:0,2,0,0", *flag)
    assert matrix == [0.5, 0.0, 0.0, 1.0, 0.0, 2.0, 0.0, 0.0] and sweep_of(said)[3] == [0.0, 45.0]


def test_sweep_combines_with_the_steps_julia_and_the_run_flags(exe, tmp_path):
    matrix, said = stated(exe, tmp_path, "--sweep", "zi,cr:0:90:8", "--julia", "-0.8,0.156", "--power", "3", *RUN_FLAGS)
    assert matrix == IDENTITY
    assert [float.fromhex(v) for v in said.pop("julia")] == [-0.8, 0.156] and said.pop("power") == 3
    assert len(sweep_of(said)[3]) == 8
    _, said = stated(exe, tmp_path, "--formula", "buffalo", "--sweep", "zi,cr:0:90:8", "--tonemap", "thresholds")
    assert said.pop("formula") == "buffalo" and len(sweep_of(said)[3]) == 8
    _, said = stated(exe, tmp_path, "--burning-ship", "--sweep", "zi,cr:0:90:8", "--state-format", "native")
    assert list(said) == ["sweep"]


def test_without_the_flag_no_sweep_line(exe, tmp_path):
    r = run(exe, *SMALL, "--plane", "zr,cr", cwd=tmp_path)
    assert "sweep" not in r.stderr and "projection" in r.stderr.split("\n")[0]
