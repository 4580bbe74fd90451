"""The `cudabrot` binary's --equalize flag without a GPU, in the manner of tests/test_exposure_cli.py: the flag parses with
every render family, its two refusals print their line, the usage text and exit 0 with nothing written, the usage text
names the flag among the output options, and --stats states it before any device is touched."""

import json
import os

import pytest

from cli_harness import CHANNELS, refused, run, stats_lines
from cli_harness import exe  # noqa: F401 (a fixture)

WITH_CLIP = "--equalize does not combine with --white-clip."
WITH_COLOR = "--equalize does not combine with --color."
COLOR = ["--color", "c.ppm"]


@pytest.mark.parametrize(
    "args,first_line",
    # the two refusals, in both orders of the flags; the table's last rows: every older row speaks first
    [(["--equalize", "--white-clip", "1"], WITH_CLIP), (["--white-clip", "0x1p-1", "--equalize"], WITH_CLIP),
     (CHANNELS + COLOR + ["--equalize"], WITH_COLOR), (["--equalize"] + CHANNELS + COLOR, WITH_COLOR),
     (["--bounded", "--equalize", "--white-clip", "0.1", "-w", "16"], WITH_CLIP),
     (CHANNELS + COLOR + ["--equalize", "--white-clip", "1"], "--white-clip does not combine with --color."),
     (CHANNELS + COLOR + ["--equalize", "--density-filter", "4"], "--density-filter does not combine with --color."),
     (["--equalize"] + COLOR, "--color needs exactly 3 --channel images, got 0."),
     (COLOR + CHANNELS + ["--equalize", "--anti"], "--anti does not combine with --channel.")],
)
def test_equalize_refusals_print_message_then_usage_and_exit_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


def test_help_lists_the_flag_after_the_density_filter(exe):
    out = run(exe, "--help").stdout
    assert "  --equalize: " in out
    assert out.index("--density-filter") < out.index("--equalize") < out.index("The following settings control the location")
    assert out.rstrip().split("\n")[-1] == "             include in the output image. Defaults to 2.0."


@pytest.mark.parametrize(
    "more",
    [[], ["--white-clip", "0"], ["--bounded", "--julia", "-1,0"], ["--palette", "0:ffffff"], ["--depth", "cr:-2:0.5:3"],
     ["--sweep", "zr,cr:0:90:2"], ["--bounded", "--period-palette", "0:000000,2:ffffff"], ["--anti"], CHANNELS[:4],
     ["--depth", "cr:-2:0.5:3", "--depth-palette", "0:ff0000,2:0000ff"], ["--gpus", "2"], ["--density-filter", "4"],
     ["-g", "0.5", "--tonemap", "host"], ["--tonemap", "lut"], ["--tonemap", "thresholds"]],
)
def test_the_flag_passes_the_parser_with_every_render_family(exe, more, tmp_path):
    """Accepted: the run gets as far as the device (exit 1 without a GPU, 0 with one) -- either way no usage text."""
    r = run(exe, "--equalize", *more, "-w", "8", "-h", "8", "--passes", "0", "-o", os.devnull, cwd=tmp_path)
    assert "Usage:" not in r.stdout
    assert r.stdout.startswith("Creating 8x8 image")


def test_stats_state_the_flag_before_any_device_is_touched(exe, tmp_path):
    said = [line for line in stats_lines(exe, tmp_path, "--equalize", "-o", os.devnull) if line.startswith('{"equalize"')]
    assert len(said) == 1 and json.loads(said[0]) == {"equalize": True}
    assert not any("equalize" in line for line in stats_lines(exe, tmp_path, "-o", os.devnull))
