"""The frames render without a GPU (include/cudabrot_amd.h, "Frames render"): cb_frames_from_sweep and
cb_rotate_projection, which are host arithmetic, and the restatement (tests/frames_reference.py) at F = 1."""

import ctypes as C
import math

import numpy as np
import pytest

import frames_reference as frames
import plot_reference as plot
from plot_harness import INVALID, ref  # noqa: F401  (a fixture)

AXES = plot.AXES
IDENTITY8 = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]


def sweep(cb, base, x, y, deg0, deg1, n, out=None, angles=True):
    """The raw call -> (return code, out [n, 8], angles [n])."""
    b = None if base is None else (C.c_double * 8)(*np.asarray(base, dtype=np.float64).reshape(-1))
    if out is None:
        out = np.full((max(n, 1), 8), 7.5)
    ang = np.full(max(n, 1), 7.5)
    rc = cb.lib.cb_frames_from_sweep(b, x, y, deg0, deg1, n, out.ctypes.data, ang.ctypes.data if angles else None)
    return rc, out, ang


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_a_full_turn_in_four_frames_is_exact(cb):
    m, angles = cb.frames_from_sweep(IDENTITY8, ("zr", "zi"), 0.0, 360.0, 4)
    assert list(angles) == [0.0, 90.0, 180.0, 270.0]
    # frame f: a' = a co - b si, b' = a si + b co on the columns (zr, zi) of both rows
    want = [[1, 0, 0, 0, 0, 1, 0, 0], [0, 1, 0, 0, -1, 0, 0, 0], [-1, 0, 0, 0, 0, -1, 0, 0], [0, -1, 0, 0, 1, 0, 0, 0]]
    assert np.array_equal(m, np.array(want, dtype=np.float64))
    assert not np.signbit(m[m == 0.0]).any()  # every zero is +0


@pytest.mark.parametrize("axes", [("zi", "cr"), ("cr", "zr"), (3, 1)])
def test_frame_0_of_a_sweep_from_0_is_the_base(cb, axes):
    base = plot.HOLOGRAM.reshape(-1)
    m, angles = cb.frames_from_sweep(base, axes, 0.0, 77.0, 9)
    assert angles[0] == 0.0 and np.array_equal(bits(m[0]), bits(base + 0.0))


def test_an_irrational_sweep_is_the_rotation_at_the_returned_angles(cb):
    base = plot.HOLOGRAM
    m, angles = cb.frames_from_sweep(base, ("zi", "cr"), 3.0, 100.0, 7)
    for f in range(7):
        a = 3.0 + ((100.0 - 3.0) * float(f)) / 7.0  # the three operations, in that order
        assert angles[f] == a
        assert a / 90.0 != math.floor(a / 90.0)
        assert np.array_equal(bits(m[f]), bits(plot.rotate(base, "zi", "cr", a).reshape(-1) + 0.0)), f
    # every frame from the base, never from the frame before: the last frame alone, asked for on its own angle
    one, _ = cb.frames_from_sweep(base, ("zi", "cr"), angles[6], angles[6] + 1.0, 1)
    assert np.array_equal(bits(one[0]), bits(m[6]))


def test_quarter_turns_inside_a_sweep_are_exact_and_the_rest_is_not_rounded_to_them(cb):
    m, angles = cb.frames_from_sweep(IDENTITY8, ("zi", "cr"), -90.0, 270.0, 8)
    assert list(angles) == [-90.0, -45.0, 0.0, 45.0, 90.0, 135.0, 180.0, 225.0]
    assert list(m[0]) == [1, 0, 0, 0, 0, 0, -1, 0] and list(m[4]) == [1, 0, 0, 0, 0, 0, 1, 0]
    assert list(m[6]) == [1, 0, 0, 0, 0, -1, 0, 0]
    assert m[3][5] == math.cos(45.0 * (math.pi / 180.0)) and m[3][6] == math.sin(45.0 * (math.pi / 180.0))


def test_rotate_projection_is_the_sweeps_arithmetic(cb):
    p = (C.c_double * 8)(*plot.HOLOGRAM.reshape(-1))
    assert cb.lib.cb_rotate_projection(p, AXES["zr"], AXES["ci"], 33.0) == 0
    m, _ = cb.frames_from_sweep(plot.HOLOGRAM, ("zr", "ci"), 33.0, 34.0, 1)
    assert np.array_equal(bits(list(p)), bits(m[0]))
    before = list(p)
    for x, y, deg in ((0, 0, 1.0), (-1, 1, 1.0), (0, 4, 1.0), (0, 1, float("nan")), (0, 1, float("inf"))):
        assert cb.lib.cb_rotate_projection(p, x, y, deg) == INVALID and list(p) == before
    assert cb.lib.cb_rotate_projection(None, 0, 1, 1.0) == INVALID


def test_every_refusal_leaves_out_untouched(cb):
    nan, inf = float("nan"), float("inf")
    bad_base = list(IDENTITY8)
    bad_base[6] = inf
    for args in ((IDENTITY8, 1, 1, 0.0, 90.0, 4), (IDENTITY8, -1, 1, 0.0, 90.0, 4), (IDENTITY8, 0, 4, 0.0, 90.0, 4),
                 (IDENTITY8, 0, 1, nan, 90.0, 4), (IDENTITY8, 0, 1, 0.0, inf, 4), (IDENTITY8, 0, 1, -inf, 90.0, 4),
                 (bad_base, 0, 1, 0.0, 90.0, 4), (IDENTITY8, 0, 1, 0.0, 90.0, 0), (IDENTITY8, 0, 1, 0.0, 90.0, -3),
                 (IDENTITY8, 0, 1, 0.0, 90.0, cb.CB_FRAMES_MAX + 1), (None, 0, 1, 0.0, 90.0, 4),
                 (IDENTITY8, 0, 1, -1.7e308, 1.7e308, 4)):  # the last: deg1 - deg0 is not finite
        out = np.full((cb.CB_FRAMES_MAX + 1, 8), 7.5)
        rc, out, ang = sweep(cb, *args, out=out)
        assert rc == INVALID and (out == 7.5).all() and (ang == 7.5).all(), args
    b = (C.c_double * 8)(*IDENTITY8)
    assert cb.lib.cb_frames_from_sweep(b, 0, 1, 0.0, 90.0, 4, None, None) == INVALID
    rc, out, _ = sweep(cb, IDENTITY8, 0, 1, 0.0, 90.0, cb.CB_FRAMES_MAX, out=np.zeros((cb.CB_FRAMES_MAX, 8)), angles=False)
    assert rc == 0 and out[cb.CB_FRAMES_MAX - 1].any()  # the most frames there are, and no angles asked for
    with pytest.raises(ValueError):
        cb.frames_from_sweep(IDENTITY8, ("zr", "zz"), 0.0, 1.0, 2)


def test_the_restatement_with_one_frame_is_the_projected_render(ref, oracle):
    w, h, max_iter, min_iter, threads, launches = 64, 48, 200, 2, 64, [20, 3]
    for kw in (dict(), dict(c=(-0.8, 0.156)), dict(degree=3)):
        own = oracle.init_states(1337, 0, threads)
        want, wc = plot.draw(ref, w, h, max_iter, min_iter, threads, launches, projection=plot.HOLOGRAM, states=own, **kw)
        states = oracle.init_states(1337, 0, threads)
        hist, cnt = frames.draw(ref, [plot.HOLOGRAM], w, h, max_iter, min_iter, threads, launches, states=states, **kw)
        assert hist.shape == (1, h, w) and np.array_equal(hist[0], want) and cnt == wc and wc["increments"] > 0
        assert states.tobytes() == own.tobytes()


def test_the_restatement_sums_increments_and_keeps_the_other_counters(ref):
    w, h, max_iter, min_iter, threads, launches = 64, 48, 200, 2, 64, [20]
    mats = [plot.IDENTITY, plot.HOLOGRAM, plot.plane("zr", "cr")]
    hist, cnt = frames.draw(ref, mats, w, h, max_iter, min_iter, threads, launches)
    singles = [plot.draw(ref, w, h, max_iter, min_iter, threads, launches, projection=p) for p in mats]
    assert all(np.array_equal(hist[f], singles[f][0]) for f in range(3))
    assert cnt["increments"] == sum(c["increments"] for _, c in singles) == int(hist.sum())
    assert all(cnt[k] == singles[0][1][k] for k in cnt if k != "increments")
