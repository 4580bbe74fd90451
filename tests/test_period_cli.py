"""The `cudabrot` binary's --period-palette and --period-eps flags without a GPU: messages, refusals and exit codes follow
the conventions of the other extension flags (tests/test_bounded_cli.py): message, usage, exit 0; nothing is rendered.  What
the flags mean is read from the lines that --stats prints before any device is touched."""

import pytest

from cli_harness import CHANNELS, IDENTITY, RUN_FLAGS, SMALL, refused, run, stated
from cli_harness import exe  # noqa: F401 (a fixture)

PP = ["--period-palette", "1:ff0000,2:00ff00,3:0000ff"]
BOUNDED = ["--bounded"]
BOTH = BOUNDED + PP
# (the other flags of the line, its first line); every line is tried with the flags of this file first and last
NEW_ROWS = (
    # the rows of this file, ahead of --bounded's
    (["--period-eps", "0x1p-40"], [], "--period-eps needs --period-palette."),
    (["--period-eps", "0"], BOUNDED, "--period-eps needs --period-palette."),
    (["--period-eps", "1e-20"], ["--anti"], "--period-eps needs --period-palette."),
    (PP, [], "--period-palette needs --bounded."),
    (PP + ["--period-eps", "0"], [], "--period-palette needs --bounded."),
    (PP, ["--plane", "cr,ci"], "--period-palette needs --bounded."),
    (PP, ["--julia", "-1,0", "--power", "3"], "--period-palette needs --bounded."),
    (PP, ["--anti"], "--period-palette needs --bounded."),
    (PP, ["--depth", "cr:-2:0.5:4"], "--period-palette needs --bounded."),
    (PP, ["--state-format", "raw"], "--period-palette needs --bounded."),
    (BOTH, ["--state-format", "raw"], "--period-palette does not combine with --state-format raw."),
    (BOTH, ["--state-format", "raw", "--anti"], "--period-palette does not combine with --state-format raw."),
    (BOTH + ["--period-eps", "0"], ["--state-format", "raw", "-s", "x.bin"],
     "--period-palette does not combine with --state-format raw."),
)
# everything else is refused by --bounded's row, in its name
BOUNDED_ROW = (
    (BOTH, ["--anti"], "--bounded does not combine with --anti."),
    (BOTH, ["--palette", "0:ffffff"], "--bounded does not combine with --palette."),
    (BOTH, ["--depth", "cr:-2:0.5:4"], "--bounded does not combine with --depth."),
    (BOTH, ["--depth-palette", "0:ffffff"], "--bounded does not combine with --depth-palette."),
    (BOTH, ["--sweep", "zi,cr:0:90:4"], "--bounded does not combine with --sweep."),
    (BOTH, ["--phoenix", "-0.5,0"], "--bounded does not combine with --phoenix."),
    (BOTH, ["--focus"], "--bounded does not combine with --focus."),
    (BOTH, ["--channel", "9:1:x"], "--bounded does not combine with --channel."),
    (BOTH, CHANNELS + ["--color", "c.ppm"], "--bounded does not combine with --channel."),
    (BOTH, ["--gpus", "2"], "--bounded does not combine with --gpus above 1."),
    (BOTH, ["--julia", "-1,0", "--anti"], "--bounded does not combine with --anti."),
)
# the older rows behind keep winning where they did
OLDER_ROWS = (
    (BOTH, ["--formula", "tricorn", "--power", "3"], "--formula does not combine with --power."),
    (BOTH, ["--formula", "tricorn", "--burning-ship"], "--formula does not combine with --burning-ship."),
    (BOTH, ["--power", "3", "--burning-ship"], "--power does not combine with --burning-ship."),
    (BOTH, ["--project", "1,0,0,0:0,1,0,0", "--plane", "zr,cr"], "--project does not combine with --plane or --rotate."),
)
# a bad value speaks at once, wherever it stands
BAD_VALUES = (
    (["--period-palette", "1024:ff0000"], BOUNDED,
     "Invalid period palette (want K:RRGGBB,... K ascending from 0 to 1023, at most 16 stops): 1024:ff0000"),
    (["--period-palette", "2:ff0000,1:00ff00"], BOUNDED,
     "Invalid period palette (want K:RRGGBB,... K ascending from 0 to 1023, at most 16 stops): 2:ff0000,1:00ff00"),
    (["--period-palette", "1:ff00"], BOUNDED,
     "Invalid period palette (want K:RRGGBB,... K ascending from 0 to 1023, at most 16 stops): 1:ff00"),
    (["--period-palette", ""], BOUNDED,
     "Invalid period palette (want K:RRGGBB,... K ascending from 0 to 1023, at most 16 stops): "),
    (["--period-palette", ",".join("%d:0000ff" % k for k in range(17))], BOUNDED,
     "Invalid period palette (want K:RRGGBB,... K ascending from 0 to 1023, at most 16 stops): "
     + ",".join("%d:0000ff" % k for k in range(17))),
    (BOTH + ["--period-eps", "-1"], [], "Invalid period eps (want a finite number, 0 or more): -1"),
    (BOTH + ["--period-eps", "-0x1p-1074"], [], "Invalid period eps (want a finite number, 0 or more): -0x1p-1074"),
    (BOTH + ["--period-eps", "inf"], [], "Invalid period eps (want a finite number, 0 or more): inf"),
    (BOTH + ["--period-eps", "nan"], [], "Invalid period eps (want a finite number, 0 or more): nan"),
    (BOTH + ["--period-eps", "tiny"], [], "Invalid number given to argument --period-eps: tiny"),
    (BOTH + ["--period-eps", ""], [], "Invalid number given to argument --period-eps: "),
)
ROWS = NEW_ROWS + BOUNDED_ROW + OLDER_ROWS + BAD_VALUES
REFUSED = [(a + b, line) for a, b, line in ROWS] + [(b + a, line) for a, b, line in ROWS if b]
WITH_STATS = [(["--stats"] + a + b, line) for a, b, line in ROWS]


@pytest.mark.parametrize("args,first_line", REFUSED + WITH_STATS)
def test_the_flags_print_message_then_usage_and_exit_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


@pytest.mark.parametrize("flag", ["--period-palette", "--period-eps"])
def test_the_flags_need_a_value(exe, tmp_path, flag):
    r = run(exe, "--bounded", flag, cwd=tmp_path)
    assert r.returncode == 0 and r.stdout.split("\n")[0] == "Argument %s needs a value." % flag


def test_usage_does_not_list_the_flags(exe):
    """The usage text is the reference's and lists no extension flag; README.md and DESIGN.md 4.22 describe these."""
    out = run(exe, "--help").stdout
    assert "--period-palette" not in out and "--period-eps" not in out and "period" not in out


def test_the_stats_line_stands_beside_the_bounded_line(exe, tmp_path):
    matrix, said = stated(exe, tmp_path, *BOTH)
    assert matrix == IDENTITY
    assert said == {"bounded": True, "period_palette": [[1, "ff0000"], [2, "00ff00"], [3, "0000ff"]], "period_eps": "0x1p-66"}
    assert list(said) == ["bounded", "period_palette", "period_eps"]
    r = run(exe, *SMALL, *BOTH, cwd=tmp_path)
    assert r.stderr.split("\n")[1:3] == [
        '{"bounded": true}',
        '{"period_palette": [[1, "ff0000"], [2, "00ff00"], [3, "0000ff"]], "period_eps": "0x1p-66"}']


@pytest.mark.parametrize("text,want", [("0", 0.0), ("0x1p-66", 2.0 ** -66), ("1e-20", 1e-20), ("0x1p+10", 1024.0),
                                       ("0x1.8p-3", 0.1875), ("-0", 0.0)])
def test_period_eps_takes_decimals_and_hexfloats(exe, tmp_path, text, want):
    _, said = stated(exe, tmp_path, *BOTH, "--period-eps", text)
    assert float.fromhex(said["period_eps"]) == want and list(said) == ["bounded", "period_palette", "period_eps"]


@pytest.mark.parametrize("first", ["period", "others"])
@pytest.mark.parametrize("others,keys,matrix", [
    ([], ["bounded", "period_palette"], [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]),
    (["--plane", "cr,ci"], ["bounded", "period_palette"], [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]),
    (["--plane", "zr,cr"], ["bounded", "period_palette"], [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]),
    (["--rotate", "zr,cr:90"], ["bounded", "period_palette"], [0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0]),
    (["--project", "0.5,0,0,1:0,2,0,0"], ["bounded", "period_palette"], [0.5, 0.0, 0.0, 1.0, 0.0, 2.0, 0.0, 0.0]),
    (["--power", "3", "--julia", "-0.1,0.6"], ["power", "julia", "bounded", "period_palette"],
     [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]),
    (["--formula", "tricorn"], ["formula", "bounded", "period_palette"], [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]),
    (["--burning-ship", "--julia", "-1,0"], ["julia", "bounded", "period_palette"], [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]),
    (["--period-eps", "0"], ["bounded", "period_palette"], [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]),
    (["--state-format", "native"], ["bounded", "period_palette"], [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]),
])
def test_it_combines_with_the_planes_the_steps_julia_and_the_run_flags(exe, tmp_path, others, keys, matrix, first):
    args = (PP + BOUNDED + others if first == "period" else others + BOUNDED + PP) + RUN_FLAGS
    got, said = stated(exe, tmp_path, *args)
    assert got == matrix and list(said) == keys + ["period_eps"]  # (the last line's second key)
    assert said["period_palette"] == [[1, "ff0000"], [2, "00ff00"], [3, "0000ff"]]


def test_stops_at_the_ends_of_the_range_are_taken(exe, tmp_path):
    _, said = stated(exe, tmp_path, "--bounded", "--period-palette", "0:101010,1023:ABCDEF")
    assert said["period_palette"] == [[0, "101010"], [1023, "abcdef"]]
    _, said = stated(exe, tmp_path, "--bounded", "--period-palette", "0:ffffff")  # one stop at 0: a table of two entries
    assert said["period_palette"] == [[0, "ffffff"]]


def test_without_the_flags_no_period_line(exe, tmp_path):
    r = run(exe, *SMALL, "--bounded", cwd=tmp_path)
    assert "period" not in r.stderr and r.stderr.split("\n")[1] == '{"bounded": true}'
