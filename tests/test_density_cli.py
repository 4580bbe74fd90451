"""The `cudabrot` binary's --density-filter flag without a GPU: messages, the refusal and exit codes follow the conventions
of the other extension flags (tests/test_exposure_cli.py): message, usage, exit 0; nothing is rendered.  Like --white-clip
the flag is listed in the usage text, right after it."""

import json
import os

import pytest

from cli_harness import CHANNELS, refused, run
from cli_harness import exe  # noqa: F401 (a fixture)

BAD = "Invalid density filter (want R[:ALPHA[:N0]], R from 1 to 8): "
REFUSED = "--density-filter does not combine with --color."
COLOR = ["--color", "c.ppm"]
BAD_VALUES = ("x", "0", "9", "-1", "", " 4", "4 ", "4:", "4:x", "4::1", "4:0.5:", "4:0.5:0", "4:0.5:1048577", "4:0.5:1:2",
              "4:0.01", "4:4.5", "4:nan", "4:inf", "4: 0.5", "4:0.5:-1", "4.0", "0x4", "8:0.0625", "8:0.5:65536", "4,0.5")


@pytest.mark.parametrize(
    "args,first_line",
    [(["--density-filter"], "Argument --density-filter needs a value.")]
    + [(["--density-filter", v], BAD + v) for v in BAD_VALUES]
    + [(["--bounded", "--density-filter", "9", "-w", "16"], BAD + "9")]
    # the refusal with --color, in both orders of the two flags; the table's last row: every older row speaks first
    + [(CHANNELS + COLOR + ["--density-filter", "4"], REFUSED), (["--density-filter", "2:0x1p-1:3"] + CHANNELS + COLOR, REFUSED),
       (CHANNELS + COLOR + ["--white-clip", "1", "--density-filter", "4"], "--white-clip does not combine with --color."),
       (["--density-filter", "4"] + COLOR, "--color needs exactly 3 --channel images, got 0."),
       (COLOR + CHANNELS + ["--density-filter", "4", "--anti"], "--anti does not combine with --channel.")],
)
def test_density_filter_flag_prints_message_then_usage_and_exits_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


def test_help_lists_the_flag_after_the_white_clip(exe):
    out = run(exe, "--help").stdout
    assert "  --density-filter <R[:ALPHA[:N0]]>: " in out
    assert out.index("--white-clip") < out.index("--density-filter") < out.index("The following settings control the location")
    assert out.rstrip().split("\n")[-1] == "             include in the output image. Defaults to 2.0."


def test_stats_print_the_filter_and_its_table_before_any_device_is_touched(exe, tmp_path):
    r = run(exe, "--density-filter", "8:0x1p-1", "--stats", "-w", "8", "-h", "8", "--passes", "0", "-o", os.devnull, cwd=tmp_path)
    said = [line for line in r.stderr.split("\n") if line.startswith('{"density_filter"')]
    assert len(said) == 1
    d = json.loads(said[0])["density_filter"]
    assert float.fromhex(d.pop("alpha")) == 0.5
    assert d == {"radius": 8, "n0": 1, "thresholds": [64, 16, 7, 4, 2, 1, 1, 1]}
    r = run(exe, "--stats", "-w", "8", "-h", "8", "--passes", "0", "-o", os.devnull, cwd=tmp_path)
    assert "density_filter" not in r.stderr


@pytest.mark.parametrize(
    "args",
    [["--density-filter", v] for v in ("1", "8", "4:0.5", "4:0x1p-1", "4:0.4:16", "2:0.125","8:4:1048576",
                                        "8:0.5:65535", "1:0.0625:1048576", "4:5e-1:9")]
    # with every render family, --channel, --gpus, -g, --white-clip and --tonemap
    + [["--density-filter", "4"] + more for more in (
        ["--bounded", "--julia", "-1,0"], ["--palette", "0:ffffff"], ["--depth", "cr:-2:0.5:3"], ["--sweep", "zr,cr:0:90:2"],
        ["--bounded", "--period-palette", "0:000000,2:ffffff"], ["--anti"], CHANNELS[:4], ["--gpus", "2"],
        ["-g", "2.2", "--tonemap", "host"], ["--tonemap", "thresholds"], ["--white-clip", "1"])],
)
def test_good_values_pass_the_parser_and_the_flag_after_passes_0_writes_an_image(exe, args, tmp_path):
    """Accepted: the run gets as far as the device (exit 1 without a GPU, 0 with one) -- either way no usage text; where
    there is a device, zero passes still end in an image."""
    image = tmp_path / "out.pgm"
    r = run(exe, *args, "-w", "8", "-h", "8", "--passes", "0", "-o", str(image), cwd=tmp_path)
    assert "Usage:" not in r.stdout
    assert r.stdout.startswith("Creating 8x8 image")
    if r.returncode == 0 and "--channel" not in args:
        assert image.exists() and image.stat().st_size > 8 * 8 * 2
        assert "Density filter: radius 4, alpha 0.5, n0 1 (the values above carry 8 fraction bits)" in r.stdout or args[1] != "4"
