"""The `cudabrot` binary's --local-equalize flag without a GPU, in the manner of tests/test_equalize_cli.py: the flag parses
with every render family and in every form of its value, its five refusals print their line, the usage text and exit 0 with
nothing written -- in both orders of the flags, behind every older row of the refusal table --, the usage text names the
flag after --equalize, and --stats states the grid and the clip before any device is touched."""

import json
import os

import pytest

from cli_harness import CHANNELS, both_orders, refused, run, stats_lines
from cli_harness import exe  # noqa: F401 (a fixture)

INVALID = "Invalid local equalisation (want TX[xTY][:CLIP], 1 to 16 tiles a side, CLIP 0 or from 1 to 256): "
SUBJECT = "--local-equalize does not combine with "
COLOR = ["--color", "c.ppm"]


@pytest.mark.parametrize(
    "args,first_line",
    both_orders(["--local-equalize", "4"],
                [(["--equalize"], SUBJECT + "--equalize."), (["--white-clip", "1"], SUBJECT + "--white-clip."),
                 (CHANNELS + COLOR, SUBJECT + "--color."),
                 (["-w", "3"], "--local-equalize needs a pixel per tile: 4x4 tiles on a 3x1000 image."),
                 # every older row speaks first
                 (["--equalize", "--white-clip", "1"], "--equalize does not combine with --white-clip."),
                 (COLOR, "--color needs exactly 3 --channel images, got 0."),
                 (CHANNELS + COLOR + ["--density-filter", "4"], "--density-filter does not combine with --color."),
                 (CHANNELS + ["--anti"], "--anti does not combine with --channel.")])
    + both_orders(["--local-equalize", "2x9:0"],
                  [(["-h", "8", "-w", "2"], "--local-equalize needs a pixel per tile: 2x9 tiles on a 2x8 image."),
                   # the tiles before the partners
                   (["-h", "8", "--equalize"], "--local-equalize needs a pixel per tile: 2x9 tiles on a 1000x8 image.")])
    + [(["--local-equalize", bad], INVALID + bad)
       for bad in ("0", "17", "4x0", "4x17", "x4", "4x", "4:", "4:0.5", "4:257", "4:-1", "4:nan", "4: 2", "", " 4", "4 ", "4x4x4",
                   "4:2:2", "four", "4,4", "-4", "4:0x1p9")],
)
def test_local_equalize_refusals_print_message_then_usage_and_exit_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


def test_a_missing_value_is_the_generic_line(exe, tmp_path):
    refused(exe, ["--local-equalize"], "Argument --local-equalize needs a value.", tmp_path)


def test_help_lists_the_flag_after_equalize(exe):
    out = run(exe, "--help").stdout
    assert "  --local-equalize <TX[xTY][:CLIP]>: " in out
    assert out.index("  --equalize: ") < out.index("  --local-equalize") < out.index("The following settings control the location")
    assert out.rstrip().split("\n")[-1] == "             include in the output image. Defaults to 2.0."


@pytest.mark.parametrize(
    "more",
    [[], ["--white-clip", "0"], ["--bounded", "--julia", "-1,0"], ["--palette", "0:ffffff"], ["--depth", "cr:-2:0.5:3"],
     ["--sweep", "zr,cr:0:90:2"], ["--bounded", "--period-palette", "0:000000,2:ffffff"], ["--anti"], CHANNELS[:4],
     ["--depth", "cr:-2:0.5:3", "--depth-palette", "0:ff0000,2:0000ff"], ["--gpus", "2"], ["--density-filter", "4"],
     ["-g", "0.5", "--tonemap", "host"], ["--tonemap", "lut"], ["--tonemap", "thresholds"], ["--focus"], ["--power", "3"],
     ["--formula", "celtic"], ["--phoenix", "0.5,0"], ["--aim"], ["--plane", "zr,cr"]],
)
def test_the_flag_passes_the_parser_with_every_render_family(exe, more, tmp_path):
    """Accepted: the run gets as far as the device (exit 1 without a GPU, 0 with one) -- either way no usage text."""
    r = run(exe, "--local-equalize", "4x2:2", *more, "-w", "8", "-h", "8", "--passes", "0", "-o", os.devnull, cwd=tmp_path)
    assert "Usage:" not in r.stdout
    assert r.stdout.startswith("Creating 8x8 image")


@pytest.mark.parametrize(
    "value,tiles,clip_q",
    [("4", [4, 4], 1024), ("1", [1, 1], 1024), ("16x16", [16, 16], 1024), ("3x5", [3, 5], 1024), ("4:0", [4, 4], 0),
     ("4:1", [4, 4], 256), ("2x3:256", [2, 3], 65536), ("4:2.5", [4, 4], 640), ("4:0x1.8p1", [4, 4], 768),
     ("4:1.001", [4, 4], 256), ("4:1.002", [4, 4], 257), ("08x02:2e0", [8, 2], 512)],
)
def test_stats_state_the_grid_and_the_clip_before_any_device_is_touched(exe, tmp_path, value, tiles, clip_q):
    lines = stats_lines(exe, tmp_path, "--local-equalize", value, "-o", os.devnull)
    said = [line for line in lines if line.startswith('{"local_equalize"')]
    assert len(said) == 1 and json.loads(said[0]) == {"local_equalize": {"tiles": tiles, "clip_q": clip_q}}
    assert said[0] == '{"local_equalize": {"tiles": [%d, %d], "clip_q": %d}}' % (tiles[0], tiles[1], clip_q)


def test_stats_without_the_flag_say_nothing_of_it(exe, tmp_path):
    assert not any("local_equalize" in line for line in stats_lines(exe, tmp_path, "-o", os.devnull))
    assert not any("local_equalize" in line for line in stats_lines(exe, tmp_path, "--equalize", "-o", os.devnull))
