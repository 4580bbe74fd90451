"""The anti-Buddhabrot (CB_KERNEL_FLAG_ANTI) without a GPU: the cycle compression of its definition against the naive
form on the CPU restatement (tests/anti_reference.c), the CLI's refusal of --anti with --channel, and the flag's value.

anti_reference.EDGE_M is the list of M at which the compression decides something (tests/test_gpu_anti_edges.py runs the
kernels at the same values).  The census of the restatement says how often each decision is met; the floors asserted on
it are conditions for the comparison to mean something, and the sample stream meets them with room (1088 at the least
where 1000 is asked)."""

import math
import os
import re
import subprocess

import numpy as np
import pytest

import anti_reference as anti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAME = ("samples", "rejected", "never_escaped", "too_fast", "recorded", "iterate_steps", "replay_steps", "increments")
EDGE_M = anti.EDGE_M


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


@pytest.mark.parametrize("max_iter", sorted(set(EDGE_M + [100, 20000])))
@pytest.mark.parametrize("ship", [False, True], ids=["mandelbrot", "burning_ship"])
def test_hand_picked_starting_points(ref, max_iter, ship):
    re_, im_ = hand_picked()
    naive, cn = anti.points(ref, 256, 256, max_iter, re_, im_, ship=ship, mode=anti.NAIVE)
    comp, cc, cen = anti.points(ref, 256, 256, max_iter, re_, im_, ship=ship, mode=anti.COMPRESSED, census=True)
    assert np.array_equal(naive, comp)
    assert same_counters(cn, cc)
    assert int(naive.sum()) == cn["increments"]
    if max_iter < 120:
        assert cen["cycles"] == 0 and cc["skipped_steps"] == 0
    else:  # 0, -1 and -2 (Mandelbrot: fixed point 2; ship: fixed point 2 as well) repeat bit for bit from the start
        assert cen["cycles"] >= 3 and cen["min_q"] >= 1 and cc["skipped_steps"] >= cen["cycles"], (cen, cc)
        assert cen["at_m"] >= (3 if max_iter == 120 else 0)
    one, c1 = anti.points(ref, 256, 256, max_iter, [0.0], [0.0], ship=ship)
    assert c1["never_escaped"] == 1 and int(one[128, 128]) == max(max_iter, 0) == int(one.sum())
    minus2, c2 = anti.points(ref, 256, 256, max_iter, [-2.0], [0.0], ship=ship)
    if not ship:  # z_k = 2 for every k >= 1: never escapes, lies off the canvas (col = 256)
        assert c2["never_escaped"] == 1 and c2["increments"] == 0 and int(minus2.sum()) == 0
    if max_iter >= 1000:
        assert cc["skipped_steps"] > 0  # the cycles were found


def test_period_two_weights_are_exact(ref):
    # c = -1: z_1, z_2, ... = 0, -1, 0, -1 ... ; M odd gives one more point at 0 than at -1
    for m in (120, 121, 180, 181, 1001, 20000, 20001):
        hist, cnt, cen = anti.points(ref, 256, 256, m, [-1.0], [0.0], census=True)
        assert int(hist[128, 128]) == (m + 1) // 2 and int(hist[128, 64]) == m // 2, m
        assert cnt["increments"] == m == int(hist.sum())
        # saved at 60, matched at 120: s = p = 60, at M itself for M = 120; M = 180 is matched at 120 too
        assert cen["cycles"] == 1 and cen["max_p"] == 60 and cen["at_m"] == (1 if m == 120 else 0), (m, cen)
        assert cen["min_q"] == (m - 60) // 60 and cen["rem_nonzero"] == (1 if m % 60 else 0), (m, cen)
        assert cnt["skipped_steps"] == (m - 120) + (m - 119), (m, cnt)


CANVASES = {
    "square": (256, 256, (-2.0, 2.0, -2.0, 2.0)),
    "zoom": (300, 200, (-1.9, -0.7, -0.45, 0.35)),  # deltas 0.004: not powers of two; cycle points partly off canvas
}


@pytest.mark.parametrize("threads", [4096, 1337])
@pytest.mark.parametrize("max_iter", EDGE_M)
@pytest.mark.parametrize("ship", [False, True], ids=["mandelbrot", "burning_ship"])
def test_compressed_equals_naive_at_round_chunk_and_weight_edges(ref, ship, max_iter, threads):
    """Two passes of the default sample stream (the stream of the GPU tests' gpu_anti(..., passes=2)): histograms bit for
    bit and the SAME counters between the definition and its compression, on both canvases, and the census conditions
    under which that comparison reaches the branch this M is in the list for."""
    m = max_iter
    cen = cc = None
    for name, (w, h, box) in CANVASES.items():
        args = dict(w=w, h=h, max_iter=m, n_threads=threads, passes=2, box=box, ship=ship, omp_threads=omp_threads())
        naive, cn = anti.render(ref, mode=anti.NAIVE, **args)
        comp, cc, cen_here = anti.render(ref, mode=anti.COMPRESSED, census=True, **args)
        assert np.array_equal(naive, comp), name
        assert same_counters(cn, cc), (name, cn, cc)
        assert cn["samples"] == threads * 100 and cn["skipped_steps"] == 0
        assert int(naive.sum()) == cn["increments"], name
        assert cen is None or cen == cen_here  # what is decided about a sample does not depend on the canvas
        cen = cen_here
        if m <= 0:  # nothing is tested, nothing is added; every sample counts as not escaping
            assert int(naive.sum()) == 0
            assert cn["never_escaped"] == cn["recorded"] == cn["samples"] and cn["too_fast"] == 0
            assert cn["iterate_steps"] == cn["replay_steps"] == cn["increments"] == cc["skipped_steps"] == 0
    assert cen["rem_zero"] + cen["rem_nonzero"] == cen["cycles"] >= cen["at_m"]
    if m < 120:
        assert cen["cycles"] == 0 and cc["skipped_steps"] == 0, (cen, cc)
    else:
        assert cen["cycles"] >= 1000 and cen["min_q"] >= 1 and cen["max_p"] % 60 == 0 and cen["max_p"] >= 60, cen
        assert cc["skipped_steps"] >= cen["cycles"]  # a sample with a cycle skips at least its last replay step
    if m in (120, 180, 240):
        assert cen["at_m"] >= 1000, cen
    elif m >= 120 and m % 60 == 0:
        assert cen["rem_zero"] > 0, cen
    if m in (121, 181, 241, 500, 1000):
        assert cen["rem_nonzero"] >= 1000, cen
    if m in (121, 181, 241):  # one step past a boundary: every cycle was found before the last step
        assert cen["at_m"] == 0, cen
    if m == 120:  # every cycle is found at n == M with s = p = 60: (M - n) + (M - end) = 0 + 1 steps skipped each
        assert cen["at_m"] == cen["cycles"] == cc["skipped_steps"] and cen["min_q"] == 1 and cen["max_p"] == 60, (cen, cc)


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
