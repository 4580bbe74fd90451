"""The `cudabrot` binary's --bounded flag without a GPU: messages, refusals and exit codes follow the conventions of the
other extension flags (tests/test_phoenix_cli.py): message, usage, exit 0; nothing is rendered.  What the flag means is read
from the `"projection"`, `"julia"`, ... and `"bounded"` lines that --stats prints before any device is touched."""

import pytest

from cli_harness import CHANNELS, IDENTITY, RUN_FLAGS, SMALL, both_orders, refused, run, stated
from cli_harness import exe  # noqa: F401 (a fixture)

BOUNDED = ["--bounded"]
# the row's partners, in its order
OTHERS = (
    (["--anti"], "--bounded does not combine with --anti."),
    (["--palette", "0:ffffff"], "--bounded does not combine with --palette."),
    (["--depth", "cr:-2:0.5:4"], "--bounded does not combine with --depth."),
    (["--depth", "cr:-2:0.5:4", "--depth-palette", "0:ffffff"], "--bounded does not combine with --depth."),
    (["--depth-palette", "0:ffffff"], "--bounded does not combine with --depth-palette."),
    (["--sweep", "zi,cr:0:90:4"], "--bounded does not combine with --sweep."),
    (["--phoenix", "-0.5,0"], "--bounded does not combine with --phoenix."),
    (["--focus"], "--bounded does not combine with --focus."),
    (["--focus-level", "6"], "--bounded does not combine with --focus."),
    (["--channel", "9:1:x"], "--bounded does not combine with --channel."),
    (["--color", "c.ppm"], "--bounded does not combine with --channel."),
    (CHANNELS + ["--color", "c.ppm"], "--bounded does not combine with --channel."),
    (["--gpus", "2"], "--bounded does not combine with --gpus above 1."),
    # the first partner present speaks
    (["--anti", "--palette", "0:ffffff"], "--bounded does not combine with --anti."),
    (["--focus", "--gpus", "2"], "--bounded does not combine with --focus."),
    # the row is the table's first: beside a flag it combines with, it still speaks in its own name
    (["--julia", "-1,0", "--anti"], "--bounded does not combine with --anti."),
    (["--plane", "zr,cr", "--anti"], "--bounded does not combine with --anti."),
    (["--power", "3", "--focus"], "--bounded does not combine with --focus."),
    (["--formula", "tricorn", "--gpus", "2"], "--bounded does not combine with --gpus above 1."),
    (["--burning-ship", "--palette", "0:ffffff"], "--bounded does not combine with --palette."),
)
REFUSED = both_orders(BOUNDED, OTHERS)
# What the flag combines with keeps its own refusals, in both orders.
OLDER_ROWS = (
    (["--formula", "tricorn", "--power", "3"], "--formula does not combine with --power."),
    (["--formula", "tricorn", "--burning-ship"], "--formula does not combine with --burning-ship."),
    (["--power", "3", "--burning-ship"], "--power does not combine with --burning-ship."),
    (["--project", "1,0,0,0:0,1,0,0", "--plane", "zr,cr"], "--project does not combine with --plane or --rotate."),
)
BEHIND = both_orders(BOUNDED, OLDER_ROWS)
WITH_STATS = [(BOUNDED + ["--stats"] + o, line) for o, line in OTHERS]


@pytest.mark.parametrize("args,first_line", REFUSED + BEHIND + WITH_STATS)
def test_bounded_flag_prints_message_then_usage_and_exits_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


def test_the_flag_takes_no_value(exe, tmp_path):
    r = run(exe, "--bounded", "1", cwd=tmp_path)
    assert r.returncode == 0 and r.stdout.split("\n")[0] == "Invalid argument: 1"


def test_usage_does_not_list_the_flag(exe):
    """The usage text is the reference's and lists no extension flag; README.md and DESIGN.md 4.21 describe this one."""
    assert "--bounded" not in run(exe, "--help").stdout


def test_the_flag_alone_is_the_identity_plane_with_a_sampled_c(exe, tmp_path):
    matrix, said = stated(exe, tmp_path, "--bounded")
    assert matrix == IDENTITY
    assert said == {"bounded": True}


def test_the_stats_line(exe, tmp_path):
    r = run(exe, *SMALL, "--bounded", cwd=tmp_path)
    assert r.stderr.split("\n")[1] == '{"bounded": true}'


@pytest.mark.parametrize("first", ["bounded", "others"])
@pytest.mark.parametrize("others,keys,matrix", [
    (["--plane", "zr,cr"], ["bounded"], [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]),
    (["--rotate", "zr,cr:90"], ["bounded"], [0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0]),
    (["--project", "0.5,0,0,1:0,2,0,0"], ["bounded"], [0.5, 0.0, 0.0, 1.0, 0.0, 2.0, 0.0, 0.0]),
    (["--power", "3", "--plane", "zr,cr"], ["power", "bounded"], [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]),
    (["--julia", "-1,0"], ["julia", "bounded"], [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]),
    (["--julia", "-0.123,0.745", "--power", "4"], ["power", "julia", "bounded"], [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]),
    (["--formula", "tricorn"], ["formula", "bounded"], [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]),
    (["--formula", "celtic", "--julia", "-1,0", "--plane", "zi,ci"], ["formula", "julia", "bounded"],
     [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]),
    (["--burning-ship"], ["bounded"], [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]),
    (["--burning-ship", "--julia", "-1,0"], ["julia", "bounded"], [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]),
])
def test_it_combines_with_the_planes_the_steps_julia_and_the_run_flags(exe, tmp_path, others, keys, matrix, first):
    args = (BOUNDED + others if first == "bounded" else others + BOUNDED) + RUN_FLAGS + ["--state-format", "raw"]
    got, said = stated(exe, tmp_path, *args)
    assert got == matrix and list(said) == keys and said["bounded"] is True


def test_without_the_flag_no_bounded_line(exe, tmp_path):
    r = run(exe, *SMALL, "--julia", "0.3,0", cwd=tmp_path)
    assert "bounded" not in r.stderr and "projection" in r.stderr.split("\n")[0]
