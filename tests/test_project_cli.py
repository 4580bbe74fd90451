"""The `cudabrot` binary's --project / --plane / --rotate flags without a GPU: messages, refusals and exit codes follow the
conventions of the other extension flags (tests/test_cli_contract.py): message, usage, exit 0; nothing is rendered.  The
parsed matrix is read from the `"projection"` line that --stats prints before any device is touched."""

import json
import math

import pytest

import plot_reference as plot
from cli_harness import IDENTITY, SMALL, refused, run, stats_lines
from cli_harness import exe  # noqa: F401 (a fixture)

BAD_PROJECTION = "Invalid projection (want a,b,c,d:e,f,g,h, eight finite numbers): "
BAD_PLANE = "Invalid plane (want X,Y, two different axes of zr, zi, cr, ci): "
BAD_ROTATION = "Invalid rotation (want X,Y:DEG, two different axes of zr, zi, cr, ci and a finite angle): "
NO_MIX = "--project does not combine with --plane or --rotate."
PROJECTIONS = (["--project", "1,0,0,0:0,1,0,0"], ["--plane", "zr,cr"], ["--rotate", "zr,cr:30"])
OTHERS = (
    (["--channel", "9:1:x"], "A projection does not combine with --channel."),
    (["--color", "c.ppm"], "A projection does not combine with --channel."),
    (["--anti"], "A projection does not combine with --anti."),
    (["--focus"], "A projection does not combine with --focus."),
    (["--focus-level", "6"], "A projection does not combine with --focus."),
    (["--gpus", "2"], "A projection does not combine with --gpus above 1."),
)
REFUSED = [(p + o, line) for p in PROJECTIONS for o, line in OTHERS] + [(o + p, line) for p in PROJECTIONS for o, line in OTHERS]


@pytest.mark.parametrize(
    "args,first_line",
    [
        (["--project"], "Argument --project needs a value."),
        (["--plane"], "Argument --plane needs a value."),
        (["--rotate"], "Argument --rotate needs a value."),
        (["--project", ""], BAD_PROJECTION),
        (["--project", "1,0,0,0:0,1,0"], BAD_PROJECTION + "1,0,0,0:0,1,0"),
        (["--project", "1,0,0,0:0,1,0,0,0"], BAD_PROJECTION + "1,0,0,0:0,1,0,0,0"),
        (["--project", "1,0,0,0,0,1,0,0"], BAD_PROJECTION + "1,0,0,0,0,1,0,0"),
        (["--project", "1,0,0:0,0,1,0,0"], BAD_PROJECTION + "1,0,0:0,0,1,0,0"),
        (["--project", "1,0,0,0:0,1,0,x"], BAD_PROJECTION + "1,0,0,0:0,1,0,x"),
        (["--project", "1,0,0,0:0,1,0,0x"], BAD_PROJECTION + "1,0,0,0:0,1,0,0x"),
        (["--project", "1,0,0,0:0,1,0,nan"], BAD_PROJECTION + "1,0,0,0:0,1,0,nan"),
        (["--project", "inf,0,0,0:0,1,0,0"], BAD_PROJECTION + "inf,0,0,0:0,1,0,0"),
        (["--project", "1, 0,0,0:0,1,0,0"], BAD_PROJECTION + "1, 0,0,0:0,1,0,0"),
        (["--project", "1,,0,0:0,1,0,0"], BAD_PROJECTION + "1,,0,0:0,1,0,0"),
        (["--plane", ""], BAD_PLANE),
        (["--plane", "zr"], BAD_PLANE + "zr"),
        (["--plane", "zr,zr"], BAD_PLANE + "zr,zr"),
        (["--plane", "zr,cx"], BAD_PLANE + "zr,cx"),
        (["--plane", "zr:cr"], BAD_PLANE + "zr:cr"),
        (["--plane", "zr,cr,"], BAD_PLANE + "zr,cr,"),
        (["--plane", "ZR,CR"], BAD_PLANE + "ZR,CR"),
        (["--rotate", "zr,cr:30", "--plane", "zr,cr"], "Invalid plane (--plane goes before the first --rotate): zr,cr"),
        (["--rotate", ""], BAD_ROTATION),
        (["--rotate", "zr,cr"], BAD_ROTATION + "zr,cr"),
        (["--rotate", "zr,cr:"], BAD_ROTATION + "zr,cr:"),
        (["--rotate", "zr,zr:30"], BAD_ROTATION + "zr,zr:30"),
        (["--rotate", "zr,cq:30"], BAD_ROTATION + "zr,cq:30"),
        (["--rotate", "zr,cr:30deg"], BAD_ROTATION + "zr,cr:30deg"),
        (["--rotate", "zr,cr:inf"], BAD_ROTATION + "zr,cr:inf"),
        (["--rotate", "zr,cr: 30"], BAD_ROTATION + "zr,cr: 30"),
        (["--rotate", "zr;cr:30"], BAD_ROTATION + "zr;cr:30"),
        # --project excludes the other two, in both orders
        (["--project", "1,0,0,0:0,1,0,0", "--plane", "zr,cr"], NO_MIX),
        (["--plane", "zr,cr", "--project", "1,0,0,0:0,1,0,0"], NO_MIX),
        (["--project", "1,0,0,0:0,1,0,0", "--rotate", "zr,cr:30"], NO_MIX),
        (["--rotate", "zr,cr:30", "--project", "1,0,0,0:0,1,0,0"], NO_MIX),
    ]
    + REFUSED,
)
def test_projection_flags_print_message_then_usage_and_exit_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


def test_usage_does_not_list_the_extension_flags(exe):
    out = run(exe, "--help").stdout
    assert "--project" not in out and "--plane" not in out and "--rotate" not in out


def parsed_matrix(exe, tmp_path, *args):
    """The matrix a command line means, as the binary states it (cli_harness.stated), and its eight %a texts."""
    values = json.loads(stats_lines(exe, tmp_path, *args)[0])["projection"]
    assert len(values) == 8
    return [float.fromhex(v) for v in values], values


@pytest.mark.parametrize(
    "args,want",
    [
        (["--plane", "zr,zi"], IDENTITY),
        (["--plane", "cr,ci"], [0, 0, 1, 0, 0, 0, 0, 1]),
        (["--plane", "zr,cr"], [1, 0, 0, 0, 0, 0, 1, 0]),
        (["--plane", "ci,zi"], [0, 0, 0, 1, 0, 1, 0, 0]),
        (["--project", "1,0,0,0:0,1,0,0"], IDENTITY),
        (["--project", "0x1.8p-1,-2.5e-1,1e0,0:-0x1p-3,.5,0,3"], [0.75, -0.25, 1.0, 0.0, -0.125, 0.5, 0.0, 3.0]),
        # multiples of 90 degrees: exact 0 and +-1
        (["--rotate", "zr,cr:90"], [0, 0, 1, 0, 0, 1, 0, 0]),
        (["--rotate", "zr,cr:-90"], [0, 0, -1, 0, 0, 1, 0, 0]),
        (["--rotate", "zr,cr:270"], [0, 0, -1, 0, 0, 1, 0, 0]),
        (["--rotate", "zr,cr:180"], [-1, 0, 0, 0, 0, 1, 0, 0]),
        (["--rotate", "zr,cr:-180"], [-1, 0, 0, 0, 0, 1, 0, 0]),
        (["--rotate", "zr,cr:360"], IDENTITY),
        (["--rotate", "zr,cr:-360"], IDENTITY),
        (["--rotate", "zr,cr:0"], IDENTITY),
        (["--rotate", "zr,cr:9e1"], [0, 0, 1, 0, 0, 1, 0, 0]),
        (["--rotate", "zi,ci:90"], [1, 0, 0, 0, 0, 0, 0, 1]),
        (["--rotate", "zr,zi:90"], [0, 1, 0, 0, -1, 0, 0, 0]),
        # in command-line order, from --plane
        (["--rotate", "zr,cr:90", "--rotate", "zi,ci:90"], [0, 0, 1, 0, 0, 0, 0, 1]),
        (["--rotate", "zr,cr:90", "--rotate", "cr,ci:90"], [0, 0, 0, 1, 0, 1, 0, 0]),
        (["--rotate", "cr,ci:90", "--rotate", "zr,cr:90"], [0, 0, 1, 0, 0, 1, 0, 0]),
        (["--plane", "cr,ci", "--rotate", "cr,zr:90"], [1, 0, 0, 0, 0, 0, 0, 1]),
        (["--rotate", "zr,cr:90", "--rotate", "zr,cr:90", "--rotate", "zr,cr:180"], IDENTITY),
    ],
)
def test_planes_and_quarter_turns_give_exact_matrices(exe, tmp_path, args, want):
    got, text = parsed_matrix(exe, tmp_path, *args)
    assert got == [float(x) for x in want]
    assert all(not t.startswith("-0x0") for t in text)  # an exact zero is +0


def test_a_general_rotation_uses_the_hosts_cos_and_sin(exe, tmp_path):
    got, _ = parsed_matrix(exe, tmp_path, "--rotate", "zr,cr:30", "--rotate", "zi,ci:50")
    want = plot.HOLOGRAM.reshape(-1)
    # the run is defined by the matrix the binary prints; libm's last bit may differ from Python's
    assert all(math.isclose(g, w, rel_tol=0.0, abs_tol=4 * 2.0 ** -53) for g, w in zip(got, want))
    assert got[1] == 0.0 and got[3] == 0.0 and got[4] == 0.0 and got[6] == 0.0


def test_without_a_projection_nothing_is_printed_before_the_device(exe, tmp_path):
    r = run(exe, *SMALL, cwd=tmp_path)
    assert "projection" not in r.stderr
