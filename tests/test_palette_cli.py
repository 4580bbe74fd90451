"""The `cudabrot` binary's --palette flag without a GPU: messages, refusals and exit codes follow the conventions of the
other extension flags (tests/test_julia_cli.py): message, usage, exit 0; nothing is rendered.  What the flag means is
read from the `"palette"` line that --stats prints, next to the `"projection"` line, before any device is touched."""

import os

import pytest

from cli_harness import IDENTITY, SMALL, both_orders, refused, run, stated
from cli_harness import exe  # noqa: F401 (a fixture)

BAD = "Invalid palette (want K:RRGGBB,... K ascending, at most 16 stops): "
PALETTE = ["--palette", "20:000030,60:ff8000"]
SEVENTEEN = ",".join("%d:0000%02x" % (k, k) for k in range(17))
BAD_TEXTS = ["", "20", "20:", "20:00003", "20:0000300", "20:00003g", ":000030", "x:000030", "-1:000030", "+1:000030",
             "0x10:000030", "1.5:000030", " 20:000030", "20:000030 ", "20 :000030", "20:000030,", ",20:000030",
             "20:000030,,60:ffffff", "20:000030;60:ffffff", "20:000030,20:ffffff", "60:000030,20:ffffff",
             "20:000030,60:fffff", "99999999999:000000", SEVENTEEN]
OTHERS = (
    (["--anti"], "--palette does not combine with --anti."),
    (["--focus"], "--palette does not combine with --focus."),
    (["--focus-level", "6"], "--palette does not combine with --focus."),
    (["--focus-probe", "8"], "--palette does not combine with --focus."),
    (["--focus-dilate", "2"], "--palette does not combine with --focus."),
    (["--channel", "9:1:x"], "--palette does not combine with --channel."),
    (["--color", "c.ppm"], "--palette does not combine with --channel."),
    (["--gpus", "2"], "--palette does not combine with --gpus above 1."),
    (["--state-format", "raw"], "--palette does not combine with --state-format raw."),
    (["-m", "0"], "--palette needs -m from 1 to 16777216."),
    (["-m", "-5"], "--palette needs -m from 1 to 16777216."),
)
REFUSED = both_orders(PALETTE, OTHERS)
WITH_STATS = [(PALETTE + ["--stats"] + o, line) for o, line in OTHERS] + [(o + ["--stats"] + PALETTE, line) for o, line in OTHERS]
# the flag's own refusals come before those of the step, of c and of the projection, which the same command lines trip
BEFORE_THE_OTHERS = []
for extra in (["--power", "3"], ["--julia", "0.1,0.2"], ["--plane", "zr,cr"]):
    for o, line in OTHERS[:9]:
        BEFORE_THE_OTHERS += [(PALETTE + extra + o, line), (o + extra + PALETTE, line)]
# ... and what the flag does not refuse is still refused by the others' own rules
OTHERS_RULES = [
    (PALETTE + ["--power", "3", "--burning-ship"], "--power does not combine with --burning-ship."),
    (["--project", "1,0,0,0:0,1,0,0", "--plane", "zr,zi"] + PALETTE, "--project does not combine with --plane or --rotate."),
    (PALETTE + ["--power", "9"], "Invalid power (want an integer from 3 to 8): 9"),
    (PALETTE + ["--julia", "3,0"], "Invalid julia parameter (want RE,IM, two numbers from -2 to 2): 3,0"),
]


@pytest.mark.parametrize(
    "args,first_line",
    [(["--palette"], "Argument --palette needs a value.")]
    + [(["--palette", t], BAD + t) for t in BAD_TEXTS]
    + [(["--anti", "--palette", "bad"], BAD + "bad"), (PALETTE + ["--palette", "5:12345"], BAD + "5:12345")]
    + REFUSED
    + WITH_STATS
    + BEFORE_THE_OTHERS
    + OTHERS_RULES,
)
def test_palette_flag_prints_message_then_usage_and_exits_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


@pytest.mark.parametrize("order", ["before", "after"])
def test_m_above_the_largest_table_is_refused_after_the_reference_warning(exe, order, tmp_path):
    m = ["-m", "16777217"]
    r = run(exe, *(PALETTE + m if order == "before" else m + PALETTE), cwd=tmp_path)
    lines = r.stdout.split("\n")
    assert r.returncode == 0 and r.stderr == "" and os.listdir(tmp_path) == []
    assert lines[0].startswith("Warning: Using a high number of iterations")  # -m above 60000, as without the flag
    assert lines[1] == "--palette needs -m from 1 to 16777216." and lines[2] == "Usage: %s [options]" % exe


def test_usage_does_not_list_the_flag(exe):
    assert "--palette" not in run(exe, "--help").stdout


def test_palette_alone_is_the_identity_projection_and_states_its_stops(exe, tmp_path):
    matrix, said = stated(exe, tmp_path, "--palette", "20:000030,200:ff8000,2000:ffffff", "-m", "2000")
    assert matrix == IDENTITY
    assert said == {"palette": [[20, "000030"], [200, "ff8000"], [2000, "ffffff"]]}  # no "power", no "julia"


def test_hex_digits_in_either_case_and_stops_beyond_m(exe, tmp_path):
    _, said = stated(exe, tmp_path, "--palette", "0:AbCdEf,4294967:0000FF")
    assert said["palette"] == [[0, "abcdef"], [4294967, "0000ff"]]
    assert stated(exe, tmp_path, "--palette", ",".join("%d:0000%02x" % (k, k) for k in range(16)))[1]["palette"][15] == [
        15, "00000f"]


@pytest.mark.parametrize("order", ["before", "after"])
def test_palette_combines_with_plane_step_and_c(exe, tmp_path, order):
    rest = ["--plane", "zr,cr", "--rotate", "zr,cr:90", "--power", "5", "--julia", "-0.8,0.156"]
    matrix, said = stated(exe, tmp_path, *(PALETTE + rest if order == "before" else rest + PALETTE))
    assert matrix == [0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0]
    assert said["power"] == 5 and [float.fromhex(v) for v in said["julia"]] == [-0.8, 0.156]
    assert said["palette"] == [[20, "000030"], [60, "ff8000"]]
    matrix, said = stated(exe, tmp_path, "--burning-ship", "--project", "0.5,0,0,1:0,2,0,0", *PALETTE)
    assert matrix == [0.5, 0.0, 0.0, 1.0, 0.0, 2.0, 0.0, 0.0]
    assert said["palette"] == [[20, "000030"], [60, "ff8000"]]


def test_the_last_palette_counts(exe, tmp_path):
    assert stated(exe, tmp_path, "--palette", "1:111111", "--palette", "2:222222,3:333333")[1]["palette"] == [
        [2, "222222"], [3, "333333"]]


def test_the_ends_of_the_range_of_m_are_taken(exe, tmp_path):
    for m in ("1", "16777216"):
        r = run(exe, *SMALL, "-m", m, *PALETTE, cwd=tmp_path)
        assert "Creating 16x16 image, %s max iterations." % m in r.stdout.split("\n")[:2], r.stdout


def test_without_the_flag_no_palette_line(exe, tmp_path):
    r = run(exe, *SMALL, "--julia", "0,0", cwd=tmp_path)
    assert "palette" not in r.stderr and "projection" in r.stderr.split("\n")[0]
