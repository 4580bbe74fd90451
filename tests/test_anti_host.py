"""The anti-Buddhabrot (CB_KERNEL_FLAG_ANTI) without a GPU: the cycle compression of its definition against the naive
form on the CPU restatement (tests/anti_reference.c), the CLI's refusal of --anti with --channel, and the flag's value."""

import math
import os
import re
import subprocess

import numpy as np
import pytest

import anti_reference as anti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAME = ("samples", "rejected", "never_escaped", "too_fast", "recorded", "iterate_steps", "replay_steps", "increments")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return anti.load(tmp_path_factory.mktemp("anti_ref"))


def omp_threads():
    v = os.environ.get("OMP_NUM_THREADS", "").split(",")[0].strip()
    return int(v) if v.isdigit() and int(v) > 0 else 16


def same_counters(a, b):
    return {k: a[k] for k in SAME} == {k: b[k] for k in SAME}


@pytest.mark.parametrize("ship", [False, True], ids=["mandelbrot", "burning_ship"])
def test_compressed_equals_naive_on_a_million_samples(ref, ship):
    args = dict(w=256, h=256, max_iter=2000, n_threads=4096, passes=5, ship=ship)
    naive, cn = anti.render(ref, mode=anti.NAIVE, omp_threads=omp_threads(), **args)
    comp, cc = anti.render(ref, mode=anti.COMPRESSED, omp_threads=omp_threads(), **args)
    seq, cs = anti.render(ref, mode=anti.COMPRESSED, omp_threads=0, **args)
    assert cn["samples"] == 4096 * 50 * 5 >= 10 ** 6
    assert np.array_equal(naive, comp) and np.array_equal(comp, seq)
    assert same_counters(cn, cc) and cc == cs
    assert cn["rejected"] == 0 and cn["never_escaped"] == cn["recorded"] > 0
    assert cn["never_escaped"] + cn["too_fast"] == cn["samples"]
    assert cn["replay_steps"] == 2000 * cn["recorded"]
    assert int(naive.sum()) == cn["increments"]
    assert cn["skipped_steps"] == 0 and cc["skipped_steps"] > 0
    if not ship:  # about 9.4 % of the square [-2, 2]^2 lies in the set
        assert 0.08 < cn["never_escaped"] / cn["samples"] < 0.11


def cardioid_edge(theta, scale):
    z = complex(math.cos(theta), math.sin(theta)) * 0.5
    return (z - z * z / 2.0) * scale  # c = e^it / 2 - e^2it / 4, scaled about 0


def hand_picked():
    pts = [0.0, -1.0, -2.0, complex(-0.12256116687665361, 0.74486176661974424)]  # the last: a period-3 bulb centre
    for theta in (0.3, 1.0, 2.0, 2.9):
        for eps in (-1e-12, 1e-13, 1e-12):
            pts.append(cardioid_edge(theta, 1.0 + eps))
    return np.array([complex(p).real for p in pts]), np.array([complex(p).imag for p in pts])


@pytest.mark.parametrize("max_iter", [0, 1, 2, 100, 1000, 20000])
@pytest.mark.parametrize("ship", [False, True], ids=["mandelbrot", "burning_ship"])
def test_hand_picked_starting_points(ref, max_iter, ship):
    re_, im_ = hand_picked()
    naive, cn = anti.points(ref, 256, 256, max_iter, re_, im_, ship=ship, mode=anti.NAIVE)
    comp, cc = anti.points(ref, 256, 256, max_iter, re_, im_, ship=ship, mode=anti.COMPRESSED)
    assert np.array_equal(naive, comp)
    assert same_counters(cn, cc)
    assert int(naive.sum()) == cn["increments"]
    one, c1 = anti.points(ref, 256, 256, max_iter, [0.0], [0.0], ship=ship)
    assert c1["never_escaped"] == 1 and int(one[128, 128]) == max(max_iter, 0) == int(one.sum())
    minus2, c2 = anti.points(ref, 256, 256, max_iter, [-2.0], [0.0], ship=ship)
    if not ship:  # z_k = 2 for every k >= 1: never escapes, lies off the canvas (col = 256)
        assert c2["never_escaped"] == 1 and c2["increments"] == 0 and int(minus2.sum()) == 0
    if max_iter >= 1000:
        assert cc["skipped_steps"] > 0  # the cycles were found


def test_period_two_weights_are_exact(ref):
    # c = -1: z_1, z_2, ... = 0, -1, 0, -1 ... ; M odd gives one more point at 0 than at -1
    for m in (1001, 20000, 20001):
        hist, cnt = anti.points(ref, 256, 256, m, [-1.0], [0.0])
        assert int(hist[128, 128]) == (m + 1) // 2 and int(hist[128, 64]) == m // 2, m
        assert cnt["increments"] == m


@pytest.fixture(scope="module")
def exe():
    path = os.path.join(ROOT, "cudabrot")
    if not os.access(path, os.X_OK):
        pytest.fail("./cudabrot is not built (run `make` or __graft_entry__.build())")
    return path


@pytest.mark.parametrize("args", [["--anti", "--channel", "9:1:x"], ["--channel", "9:1:x", "--anti"],
                                  ["--anti", "--color", "c.ppm"]])
def test_cli_refuses_anti_with_channels(exe, args, tmp_path):
    r = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120,
                       cwd=tmp_path)
    assert r.returncode == 0
    lines = r.stdout.split("\n")
    assert lines[0] == "--anti does not combine with --channel."
    assert lines[1] == "Usage: %s [options]" % exe
    assert not os.path.exists(tmp_path / "x")


def test_anti_flag_value_in_header_and_package():
    with open(os.path.join(ROOT, "include", "cudabrot_amd.h")) as f:
        m = re.search(r"#define CB_KERNEL_FLAG_ANTI (0x[0-9a-fA-F]+)", f.read())
    assert m and int(m.group(1), 16) == 0x400
    import cudabrot_amd

    assert cudabrot_amd.CB_KERNEL_FLAG_ANTI == 0x400
    assert "CB_KERNEL_FLAG_ANTI" in cudabrot_amd.__all__
