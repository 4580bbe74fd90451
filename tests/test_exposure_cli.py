"""The `cudabrot` binary's --white-clip flag without a GPU: messages, the refusal and exit codes follow the conventions of
the other extension flags (tests/test_cli_contract.py): message, usage, exit 0; nothing is rendered.  Unlike them the flag
is listed in the usage text, among the output options and ahead of the canvas paragraph the text ends with."""

import os

import pytest

from cli_harness import CHANNELS, refused, run
from cli_harness import exe  # noqa: F401 (a fixture)

BAD = "Invalid white clip (want a percentage from 0 to below 100): "
REFUSED = "--white-clip does not combine with --color."
COLOR = ["--color", "c.ppm"]


@pytest.mark.parametrize(
    "args,first_line",
    [(["--white-clip"], "Argument --white-clip needs a value.")]
    + [(["--white-clip", v], BAD + v) for v in ("x", "-1", "100", "nan", "", "1%", "inf", " 1", "1e3", "0x1p7", "-0x1p-1074")]
    + [(["--bounded", "--white-clip", "100", "-w", "16"], BAD + "100")]
    # the refusal with --color, in both orders of the two flags; the table's last row: every older row speaks first
    + [(CHANNELS + COLOR + ["--white-clip", "1"], REFUSED), (["--white-clip", "0x1p-1"] + CHANNELS + COLOR, REFUSED),
       (["--white-clip", "1"] + COLOR, "--color needs exactly 3 --channel images, got 0."),
       (COLOR + CHANNELS + ["--white-clip", "1", "--anti"], "--anti does not combine with --channel.")],
)
def test_white_clip_flag_prints_message_then_usage_and_exits_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


def test_help_lists_the_flag(exe):
    out = run(exe, "--help").stdout
    assert "  --white-clip <percent>: " in out
    assert out.index("--white-clip") < out.index("The following settings control the location")
    assert out.rstrip().split("\n")[-1] == "             include in the output image. Defaults to 2.0."


@pytest.mark.parametrize(
    "args",
    [["--white-clip", v] for v in ("0", "99.999999", "0x1.8p+1", "5e-1")]
    # with every render family, --channel, --gpus, -g and --tonemap
    + [["--white-clip", "0.1"] + more for more in (
        ["--bounded", "--julia", "-1,0"], ["--palette", "0:ffffff"], ["--depth", "cr:-2:0.5:3"], ["--sweep", "zr,cr:0:90:2"],
        ["--bounded", "--period-palette", "0:000000,2:ffffff"], ["--anti"], CHANNELS[:4], ["--gpus", "2"],
        ["-g", "2.2", "--tonemap", "host"], ["--tonemap", "thresholds"])]
    + [CHANNELS + COLOR + ["--white-clip", "0"]],  # a clip of 0 is no clip
)
def test_good_values_pass_the_parser(exe, args, tmp_path):
    """Accepted: the run gets as far as the device (exit 1 without a GPU, 0 with one) -- either way no usage text."""
    r = run(exe, *args, "-w", "8", "-h", "8", "--passes", "0", "-o", os.devnull, cwd=tmp_path)
    assert "Usage:" not in r.stdout
    assert r.stdout.startswith("Creating 8x8 image")
