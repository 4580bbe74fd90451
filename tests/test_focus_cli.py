"""The `cudabrot` binary's --focus flags without a GPU: messages, refusals and exit codes follow the conventions of the
other extension flags (tests/test_cli_contract.py): message, usage, exit 0; nothing is rendered."""

import pytest

from cli_harness import refused, run
from cli_harness import exe  # noqa: F401 (a fixture)


@pytest.mark.parametrize(
    "args,first_line",
    [
        (["--focus-level"], "Argument --focus-level needs a value."),
        (["--focus-probe"], "Argument --focus-probe needs a value."),
        (["--focus-dilate"], "Argument --focus-dilate needs a value."),
        (["--focus-level", "8x"], "Invalid number given to argument --focus-level: 8x"),
        (["--focus-probe", ""], "Invalid number given to argument --focus-probe: "),
        (["--focus-dilate", "1.5"], "Invalid number given to argument --focus-dilate: 1.5"),
        (["--focus-level", "3"], "Invalid focus level (want 4 to 10): 3"),
        (["--focus-level", "11"], "Invalid focus level (want 4 to 10): 11"),
        (["--focus-probe", "0"], "Invalid focus probe (want at least 1 pass): 0"),
        (["--focus-dilate", "-1"], "Invalid focus dilation (want 0 or more cells): -1"),
        # refused combinations, in any order; each of the value flags turns --focus on
        (["--focus", "--channel", "9:1:x"], "--focus does not combine with --channel."),
        (["--channel", "9:1:x", "--focus"], "--focus does not combine with --channel."),
        (["--focus", "--color", "c.ppm"], "--focus does not combine with --channel."),
        (["--focus-level", "6", "--channel", "9:1:x"], "--focus does not combine with --channel."),
        (["--focus", "--anti"], "--focus does not combine with --anti."),
        (["--anti", "--focus-dilate", "2"], "--focus does not combine with --anti."),
        (["--focus", "--gpus", "2"], "--focus does not combine with --gpus above 1."),
        (["--gpus", "8", "--focus-probe", "4"], "--focus does not combine with --gpus above 1."),
    ],
)
def test_focus_flags_print_message_then_usage_and_exit_zero(exe, args, first_line, tmp_path):
    refused(exe, args, first_line, tmp_path)


def test_usage_does_not_list_the_extension_flags(exe):
    assert "--focus" not in run(exe, "--help").stdout
