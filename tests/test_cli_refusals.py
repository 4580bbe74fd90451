"""The order of the `cudabrot` binary's refusals, pinned on a recording -- without a GPU.

A command line that the parser refuses is answered with one message, the usage text and exit 0, and where two refusals
apply the first in the parser's order wins: `--plane zr,cr --anti --channel 9:1:x` is the projection's refusal of
--channel, `--julia 0,0 --anti --channel 9:1:x` is --julia's refusal of --anti.  That order is observable and is data
(cudabrot_amd/csrc/cli_args.cpp, the refusal table); tests/golden/cli_refusals.json holds what the binary answered to
every command line generated below BEFORE the parser was folded into that table, as tests/golden/round_kernel_counters.json
was recorded before its fold: the distinct first lines, and per command line the index of its first line, or -1 where
it was not refused (it went on to the device).  The command lines are generated anew here, the refused ones are
replayed; they touch no device.

`python tests/test_cli_refusals.py BINARY` records the file anew from that binary.
"""

import itertools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cli_refusals.json")

GOOD = [
    ["--formula", "tricorn"],
    ["--palette", "0:ffffff"],
    ["--power", "3"],
    ["--julia", "0.3,0"],
    ["--project", "1,0,0,0:0,1,0,0"],
    ["--plane", "zr,cr"],
    ["--rotate", "zr,cr:90"],
    ["--focus"],
    ["--focus-level", "6"],
    ["--anti"],
    ["--burning-ship"],
    ["--channel", "9:1:x"],
    ["--color", "c.ppm"],
    ["--gpus", "2"],
    ["--state-format", "raw"],
    ["-m", "0"],
]
BAD = [
    ["--power", "9"],
    ["--formula", "x"],
    ["--julia", "3,0"],
    ["--palette", "zz"],
    ["--focus-level", "99"],
    ["--compose", "xyz"],
    ["--channel", "a:b:c"],
    ["--state-format", "json"],
    ["--rotate", "zr,zr:1"],
    ["--bogus"],
]
FRAGMENTS = GOOD + BAD
MODES = GOOD[:10]
PARTNERS = [["--power", "3"], ["--focus"], ["--anti"], ["--burning-ship"], ["--channel", "9:1:x"], ["--color", "c.ppm"],
            ["--gpus", "2"], ["--state-format", "raw"], ["-m", "0"]]
PREFIX = ["--passes", "0", "-w", "16", "-h", "16", "-o", os.devnull]


def command_lines():
    """Every generated command line as a list of fragments, in the order the recording keeps: every ordered pair of
    distinct fragments, then for every mode m and every pair {a, b} of its partners the lines m a b and b a m."""
    lines = [[a, b] for a, b in itertools.permutations(FRAGMENTS, 2)]
    for m in MODES:
        for a, b in itertools.combinations([p for p in PARTNERS if p != m], 2):
            lines += [[m, a, b], [b, a, m]]
    return lines


def argv_of(line):
    return PREFIX + [word for fragment in line for word in fragment]


def run(exe, line, cwd=None):
    return subprocess.run([exe] + argv_of(line), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120,
                          cwd=cwd)


def record_golden(exe, path=GOLDEN):
    """What `exe` answers to every generated command line, written to `path`."""
    messages, answers = [], []
    for line in command_lines():
        r = run(exe, line)
        out = r.stdout.split("\n")
        if r.returncode == 0 and len(out) > 1 and out[1].startswith("Usage: "):
            if out[0] not in messages:
                messages.append(out[0])
            answers.append(messages.index(out[0]))
        else:
            answers.append(-1)
    with open(path, "w") as f:
        json.dump({"messages": messages, "answers": answers}, f, separators=(",", ":"))
        f.write("\n")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert len(g["answers"]) == len(command_lines()), "the recording is of another generation: record it anew"
    return g


@pytest.fixture(scope="module")
def exe():
    path = os.path.join(ROOT, "cudabrot")
    if not os.access(path, os.X_OK):
        pytest.fail("./cudabrot is not built (run `make` or __graft_entry__.build())")
    return path


@pytest.mark.parametrize("lead", range(len(FRAGMENTS)), ids=[" ".join(f) for f in FRAGMENTS])
def test_refused_command_lines_get_the_recorded_message(exe, golden, lead, tmp_path):
    replayed = 0
    for line, answer in zip(command_lines(), golden["answers"]):
        if line[0] != FRAGMENTS[lead] or answer < 0:
            continue
        r = run(exe, line, cwd=tmp_path)
        out = r.stdout.split("\n")
        assert out[0] == golden["messages"][answer], argv_of(line)
        assert out[1] == "Usage: %s [options]" % exe, argv_of(line)
        assert r.returncode == 0, argv_of(line)
        assert r.stderr == "", argv_of(line)
        assert os.listdir(tmp_path) == [], argv_of(line)
        replayed += 1
    assert replayed > 0


def combination_messages():
    """Every refusal of a combination that the parser can print, from its table."""
    rows = [
        ("--formula", ["--power", "--burning-ship", "--anti", "--focus", "--channel", "--gpus above 1"]),
        ("--palette", ["--anti", "--focus", "--channel", "--gpus above 1", "--state-format raw"]),
        ("--power", ["--burning-ship", "--anti", "--focus", "--channel", "--gpus above 1"]),
        ("--julia", ["--anti", "--focus", "--channel", "--gpus above 1"]),
        ("--project", ["--plane or --rotate"]),
        ("A projection", ["--channel", "--anti", "--focus", "--gpus above 1"]),
        ("--focus", ["--channel", "--anti", "--gpus above 1"]),
        ("--anti", ["--channel"]),
    ]
    said = ["%s does not combine with %s." % (subject, partner) for subject, partners in rows for partner in partners]
    return said + ["--palette needs -m from 1 to 16777216.", "--color needs exactly 3 --channel images, got 0.",
                   "--color needs exactly 3 --channel images, got 1."]


def test_recording_reaches_every_refusal(golden):
    """The recording is worth what it reaches: every combination refusal, the message of every bad fragment, and few
    command lines that are not refused at all."""
    bad = [
        "Invalid power (want an integer from 3 to 8): 9",
        "Invalid formula (want tricorn, celtic, buffalo, perpendicular or celtic-tricorn): x",
        "Invalid julia parameter (want RE,IM, two numbers from -2 to 2): 3,0",
        "Invalid palette (want K:RRGGBB,... K ascending, at most 16 stops): zz",
        "Invalid focus level (want 4 to 10): 99",
        "Invalid compose mode (want rgb or hsl): xyz",
        "Invalid channel (want MAX:MIN:FILE, at most 4 of them): a:b:c",
        "Invalid state format (want native or raw): json",
        "Invalid rotation (want X,Y:DEG, two different axes of zr, zi, cr, ci and a finite angle): zr,zr:1",
        "Invalid argument: --bogus",
        "Invalid plane (--plane goes before the first --rotate): zr,cr",  # (two good fragments in the wrong order)
    ]
    assert sorted(golden["messages"]) == sorted(combination_messages() + bad)
    assert len(golden["messages"]) == 43
    assert 5 * golden["answers"].count(-1) < len(golden["answers"])


if __name__ == "__main__":
    record_golden(sys.argv[1])
