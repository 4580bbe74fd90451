"""The `cudabrot` binary's --aim flags without a GPU: messages, refusals and exit codes follow the conventions of the other
extension flags (tests/test_bounded_cli.py): message, usage, exit 0; nothing is rendered.  What the flags mean is read from
the `"projection"`, `"julia"`, `"bounded"`, ... and `"aim"` lines that --stats prints before any device is touched."""

import pytest

from cli_harness import CHANNELS, IDENTITY, RUN_FLAGS, SMALL, both_orders, refused, run, stated
from cli_harness import exe  # noqa: F401 (a fixture)

AIM = ["--aim"]
# the row's partners, in its order
OTHERS = (
    (["--focus"], "--aim does not combine with --focus."),
    (["--focus-level", "6"], "--aim does not combine with --focus."),
    (["--anti"], "--aim does not combine with --anti."),
    (["--palette", "0:ffffff"], "--aim does not combine with --palette."),
    (["--bounded", "--period-palette", "0:ffffff"], "--aim does not combine with --period-palette."),
    (["--period-palette", "0:ffffff"], "--aim does not combine with --period-palette."),
    (["--depth", "cr:-2:0.5:4"], "--aim does not combine with --depth."),
    (["--depth", "cr:-2:0.5:4", "--depth-palette", "0:ffffff"], "--aim does not combine with --depth."),
    (["--depth-palette", "0:ffffff"], "--aim does not combine with --depth-palette."),
    (["--sweep", "zi,cr:0:90:4"], "--aim does not combine with --sweep."),
    (["--phoenix", "-0.5,0"], "--aim does not combine with --phoenix."),
    (["--channel", "9:1:x"], "--aim does not combine with --channel."),
    (["--color", "c.ppm"], "--aim does not combine with --channel."),
    (CHANNELS + ["--color", "c.ppm"], "--aim does not combine with --channel."),
    (["--gpus", "2"], "--aim does not combine with --gpus above 1."),
    # the first partner present speaks, in the row's order
    (["--gpus", "2", "--anti", "--focus"], "--aim does not combine with --focus."),
    (["--palette", "0:ffffff", "--anti"], "--aim does not combine with --anti."),
    (["--phoenix", "-0.5,0", "--sweep", "zi,cr:0:90:4"], "--aim does not combine with --sweep."),
    (["--gpus", "2", "--channel", "9:1:x"], "--aim does not combine with --channel."),
    # the row is the table's first: beside a flag it combines with, it still speaks in its own name
    (["--bounded", "--anti"], "--aim does not combine with --anti."),
    (["--bounded", "--focus"], "--aim does not combine with --focus."),
    (["--julia", "-1,0", "--anti"], "--aim does not combine with --anti."),
    (["--plane", "zr,cr", "--focus"], "--aim does not combine with --focus."),
    (["--power", "3", "--gpus", "2"], "--aim does not combine with --gpus above 1."),
    (["--formula", "tricorn", "--palette", "0:ffffff"], "--aim does not combine with --palette."),
    (["--burning-ship", "--depth", "cr:-2:0.5:4"], "--aim does not combine with --depth."),
)
FORMS = (AIM, ["--aim-level", "6"], ["--aim-probe", "8"], ["--aim-dilate", "0"])  # each value flag turns --aim on
REFUSED = both_orders(AIM, OTHERS)
VALUE_FLAGS = [(form + o, line) for form in FORMS[1:] for o, line in OTHERS[:3]]
# What the flag combines with keeps its own refusals, in both orders.
OLDER_ROWS = (
    (["--formula", "tricorn", "--power", "3"], "--formula does not combine with --power."),
    (["--formula", "tricorn", "--burning-ship"], "--formula does not combine with --burning-ship."),
    (["--power", "3", "--burning-ship"], "--power does not combine with --burning-ship."),
    (["--project", "1,0,0,0:0,1,0,0", "--plane", "zr,cr"], "--project does not combine with --plane or --rotate."),
    (["--period-eps", "0"], "--period-eps needs --period-palette."),
)
BEHIND = both_orders(AIM, OLDER_ROWS)
WITH_STATS = [(AIM + ["--stats"] + o, line) for o, line in OTHERS]


@pytest.mark.parametrize("args,first_line", REFUSED + VALUE_FLAGS + BEHIND + WITH_STATS)
def test_aim_flag_prints_message_then_usage_and_exits_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


@pytest.mark.parametrize("args,first_line", [
    (["--aim-level", "3"], "Invalid aim level (want 4 to 10): 3"),
    (["--aim-level", "11"], "Invalid aim level (want 4 to 10): 11"),
    (["--aim-level", "x"], "Invalid number given to argument --aim-level: x"),
    (["--aim-level"], "Argument --aim-level needs a value."),
    (["--aim-probe", "0"], "Invalid aim probe (want at least 1 pass): 0"),
    (["--aim-probe", "-3"], "Invalid aim probe (want at least 1 pass): -3"),
    (["--aim-probe"], "Argument --aim-probe needs a value."),
    (["--aim-dilate", "-1"], "Invalid aim dilation (want 0 or more cells): -1"),
    (["--aim-dilate", "1.5"], "Invalid number given to argument --aim-dilate: 1.5"),
    (["--aim", "1"], "Invalid argument: 1"),  # the flag takes no value
])
def test_value_checks(exe, tmp_path, args, first_line):
    r = run(exe, *args, cwd=tmp_path)
    assert r.returncode == 0 and r.stderr == ""
    lines = r.stdout.split("\n")
    assert lines[0] == first_line and lines[1] == "Usage: %s [options]" % exe


def test_usage_does_not_list_the_flag(exe):
    """The usage text is the reference's and lists no extension flag; README.md and DESIGN.md 4.23 describe this one."""
    assert "--aim" not in run(exe, "--help").stdout


@pytest.mark.parametrize("form,aim", [
    (AIM, {"level": 8, "probe": 64, "dilate": 1}),
    (["--aim-level", "6"], {"level": 6, "probe": 64, "dilate": 1}),
    (["--aim-probe", "8"], {"level": 8, "probe": 8, "dilate": 1}),
    (["--aim-dilate", "0"], {"level": 8, "probe": 64, "dilate": 0}),
    (["--aim-level", "4", "--aim-probe", "1", "--aim-dilate", "3", "--aim"], {"level": 4, "probe": 1, "dilate": 3}),
    (["--aim-level", "10"], {"level": 10, "probe": 64, "dilate": 1}),
])
def test_alone_it_is_the_identity_projected_render_aimed(exe, tmp_path, form, aim):
    matrix, said = stated(exe, tmp_path, *form)
    assert matrix == IDENTITY
    assert said == {"aim": aim}


@pytest.mark.parametrize("first", ["aim", "others"])
@pytest.mark.parametrize("others,keys,matrix", [
    (["--plane", "zr,cr"], ["aim"], [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]),
    (["--rotate", "zr,cr:90"], ["aim"], [0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0]),
    (["--project", "0.5,0,0,1:0,2,0,0"], ["aim"], [0.5, 0.0, 0.0, 1.0, 0.0, 2.0, 0.0, 0.0]),
    (["--power", "3", "--plane", "zr,cr"], ["power", "aim"], [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]),
    (["--julia", "-1,0"], ["julia", "aim"], IDENTITY),
    (["--formula", "tricorn"], ["formula", "aim"], IDENTITY),
    (["--burning-ship"], ["aim"], IDENTITY),
    (["--bounded"], ["bounded", "aim"], IDENTITY),
    (["--bounded", "--plane", "zr,cr"], ["bounded", "aim"], [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]),
    (["--bounded", "--julia", "-1,0"], ["julia", "bounded", "aim"], IDENTITY),
    (["--bounded", "--formula", "tricorn", "--plane", "zr,cr"], ["formula", "bounded", "aim"],
     [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]),
    (["--bounded", "--burning-ship", "--julia", "-1,0", "--plane", "zi,ci"], ["julia", "bounded", "aim"],
     [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]),
])
def test_it_combines_with_the_planes_the_steps_julia_bounded_and_the_run_flags(exe, tmp_path, others, keys, matrix, first):
    args = (AIM + others if first == "aim" else others + AIM) + RUN_FLAGS + ["--state-format", "raw"]
    got, said = stated(exe, tmp_path, *args)
    assert got == matrix and list(said) == keys and said["aim"] == {"level": 8, "probe": 64, "dilate": 1}


def test_without_the_flag_no_aim_line(exe, tmp_path):
    r = run(exe, *SMALL, "--bounded", cwd=tmp_path)
    assert "aim" not in r.stderr and "projection" in r.stderr.split("\n")[0]
