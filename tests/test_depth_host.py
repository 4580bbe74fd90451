"""The depth render without a GPU (include/cudabrot_amd.h, "Depth render"): the depth sink of the CPU restatement
(tests/plot_reference.c) against the same restatement without a depth and against the definition by hand, the header's
text, and the validation of cb_depth where it needs no device."""

import ctypes as C
import math
import os

import numpy as np
import pytest

import plot_reference as plot
from plot_harness import INVALID, ref  # noqa: F401  (a fixture)


# ---- 1. the depth sink against the restatement without a depth -----------------------------------------------------

# Every visited coordinate of a degree-2 step is below 8 + 2 sqrt 2 in magnitude, of degree 3 below (2 sqrt 2)^3 +
# 2 sqrt 2; a row of the hologram has entries of magnitude at most 1 and two of them non-zero per axis pair, so [-64, 64)
# holds it as well.
COVERING = {
    "cr_37_slices": dict(depth=("cr", -16.0, 16.0, 37)),
    "zi_64_slices": dict(depth=("zi", -16.0, 16.0, 64)),
    "hologram_row_101_slices": dict(depth=(plot.rotate(plot.IDENTITY, "zr", "ci", 37.0)[0], -64.0, 64.0, 101),
                                  projection=plot.HOLOGRAM),
    "ship": dict(depth=("zr", -16.0, 16.0, 48), ship=True),
    "power_3": dict(depth=("zi", -32.0, 32.0, 64), degree=3),
    "tricorn": dict(depth=("ci", -16.0, 16.0, 24), formula=1),
    "julia_z": dict(depth=("zr", -16.0, 16.0, 64), c=(-0.8, 0.156)),
    "julia_c": dict(depth=("cr", -16.0, 16.0, 64), c=(-0.8, 0.156)),
}


@pytest.mark.parametrize("case", list(COVERING))
def test_planes_sum_to_the_projected_render_when_the_window_covers(ref, oracle, case):
    kw = dict(COVERING[case])
    d = kw.pop("depth")
    w, h, max_iter, min_iter, threads, launches = 64, 48, 200, 2, 64, [20, 3]
    own = oracle.init_states(1337, 0, threads)
    want, wc = plot.draw(ref, w, h, max_iter, min_iter, threads, launches, states=own, **kw)
    states = oracle.init_states(1337, 0, threads)
    hist, cnt = plot.draw(ref, w, h, max_iter, min_iter, threads, launches, depth=d, states=states, **kw)
    assert wc["recorded"] > 0 and wc["increments"] > 0
    assert hist.shape == (d[3], h, w)
    assert np.array_equal(hist.sum(axis=0), want)
    assert cnt == wc and states.tobytes() == own.tobytes()
    if "c" not in kw or not (isinstance(d[0], str) and d[0].startswith("c")):
        assert sum(bool(p.any()) for p in hist) >= 2  # the points do spread over slices
    else:
        assert sum(bool(p.any()) for p in hist) == 1  # a fixed c on a c axis: one depth for every point


def test_one_slice_with_a_covering_window_is_the_projected_render(ref):
    want, wc = plot.draw(ref, 64, 48, 200, 2, 64, [20], projection=plot.ZR_CR)
    hist, cnt = plot.draw(ref, 64, 48, 200, 2, 64, [20], depth=("zi", -16.0, 16.0, 1), projection=plot.ZR_CR)
    assert hist.shape == (1, 48, 64) and np.array_equal(hist[0], want) and cnt == wc


def test_a_narrow_window_drops_points_and_only_increments_notices(ref):
    want, wc = plot.draw(ref, 64, 48, 200, 2, 64, [20])
    hist, cnt = plot.draw(ref, 64, 48, 200, 2, 64, [20], depth=("ci", -0.02, 0.02, 1))
    assert 0 < cnt["increments"] < wc["increments"] and int(hist.sum()) == cnt["increments"]
    assert {k: v for k, v in cnt.items() if k != "increments"} == {k: v for k, v in wc.items() if k != "increments"}
    assert np.all(hist[0] <= want)


def test_result_does_not_depend_on_the_thread_count(ref, oracle):
    got = []
    for omp in (0, 4):
        states = oracle.init_states(1337, 0, 256)
        hist, cnt = plot.draw(ref, 33, 17, 300, 0, 256, [50, 7], depth=("cr", -2.0, 0.5, 5), omp_threads=omp, states=states)
        got.append((hist, cnt, states.tobytes()))
    assert got[0][1]["increments"] > 100
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1] and got[0][2] == got[1][2]


# ---- 2. the definition by hand ----------------------------------------------------------------------------------------


def by_hand(d, lo, hi, n):
    """The definition in Python's IEEE doubles: early-out, truncation, bounds."""
    if d < lo:
        return None
    s = int((d - lo) / ((hi - lo) / float(n)))
    return s if 0 <= s < n else None


@pytest.mark.parametrize("lo, hi, n", [(-2.0, 2.0, 4), (-2.0, 0.5, 5), (-0.02, 0.02, 1), (0.1, 0.7, 256), (-16.0, 16.0, 64)])
def test_planted_depths_land_where_the_definition_says(ref, lo, hi, n):
    delta = (hi - lo) / float(n)
    dyadic = math.frexp(delta)[0] == 0.5
    assert plot.slice_of(ref, lo, lo, hi, n) == 0  # exactly at min: in, slice 0
    assert plot.slice_of(ref, math.nextafter(lo, -math.inf), lo, hi, n) is None  # just below min: the early-out
    assert plot.slice_of(ref, hi, lo, hi, n) == by_hand(hi, lo, hi, n)
    below_max = math.nextafter(hi, -math.inf)
    assert plot.slice_of(ref, below_max, lo, hi, n) == by_hand(below_max, lo, hi, n)
    for s in range(n):
        edge = lo + s * delta
        assert plot.slice_of(ref, edge, lo, hi, n) == by_hand(edge, lo, hi, n)
        inside = lo + (s + 0.5) * delta
        assert plot.slice_of(ref, inside, lo, hi, n) == s
        # one ulp below an edge: d - min is a rounded difference, so the neighbour of an edge may still reach the edge's
        # slice (-7.5 - ulp in [-16, 16) / 64: d - min rounds to 8.5); the definition says which, not the real line
        near = math.nextafter(edge, -math.inf)
        assert plot.slice_of(ref, near, lo, hi, n) == by_hand(near, lo, hi, n)
        if dyadic:  # every edge and every quotient is exact: the slice begins at its edge
            assert plot.slice_of(ref, edge, lo, hi, n) == s
    if dyadic:
        assert plot.slice_of(ref, hi, lo, hi, n) is None  # max itself is out
    assert plot.slice_of(ref, math.nan, lo, hi, n) is None  # !(d < min) lets it through, the bounds test does not
    assert plot.slice_of(ref, 1e300, lo, hi, n) is None and plot.slice_of(ref, -1e300, lo, hi, n) is None


def test_depth_of_a_point(ref):
    z, c = (0.3, -0.7), (-1.25, 0.4)
    for j, axis in enumerate(("zr", "zi", "cr", "ci")):
        assert plot.depth_of(ref, axis, *z, *c) == (z + c)[j]
    # the same fused operations as u: a row of the matrix and the depth row give the same number
    row = plot.HOLOGRAM[1]
    assert plot.depth_of(ref, row, *z, *c) == plot.point(ref, np.vstack([row, row]), *z, *c)[0]


# ---- 3. the header and the package ------------------------------------------------------------------------------------


def test_header_section_and_names(cb, repo_root):
    import cudabrot_amd.capi as capi

    with open(os.path.join(repo_root, "include", "cudabrot_amd.h")) as f:
        text = f.read()
    start = text.index("Depth render: the 4-D set sliced along a third axis")
    section = text[start:text.index("---- Renderer:", start)]
    for phrase in ("K_d = fma(D[2], c_re, D[3] * c_im)", "d   = fma(D[0], z_re, fma(D[1], z_im, K_d))",
                   "delta_d = (max - min) / (double) N", "!(d < min)", "s = (int) ((d - min) / delta_d)", "0 <= s < N",
                   "No table", "#define CB_DEPTH_MAX_SLICES 256", "double row[4];", "double min, max;", "int slices;",
                   "} cb_depth;"):
        assert phrase in section, phrase
    for name in ("cb_draw_buddhabrot_depth", "cb_renderer_set_depth", "cb_renderer_depth", "cb_renderer_depth_image"):
        assert name + "(" in text and name in capi.EXPORTED_SYMBOLS and hasattr(cb.lib, name)
    assert "18 the depth\n * product kernel" in text and "19 the depth lock-step kernel" in text
    assert cb.CB_DEPTH_MAX_SLICES == 256 and C.sizeof(cb.Depth) == 56
    assert callable(cb.draw_buddhabrot_depth)
    assert all(hasattr(cb.Renderer, n) for n in ("set_depth", "depth", "depth_image"))
    assert cb.lib.cb_abi_version() == 1  # the change only adds


def test_depth_make(cb):
    assert cb.Depth.make("ci", -0.02, 0.02).as_tuple() == ((0.0, 0.0, 0.0, 1.0), -0.02, 0.02, 1)
    assert cb.Depth.make([1, 2, 3, 4], 0, 1, 64).as_tuple() == ((1.0, 2.0, 3.0, 4.0), 0.0, 1.0, 64)
    with pytest.raises(ValueError):
        cb.Depth.make("xx", 0, 1)
    with pytest.raises(ValueError):
        cb.Depth.make([1, 2, 3], 0, 1)


# ---- 4. validation that needs no device -------------------------------------------------------------------------------

NAN, INF = math.nan, math.inf
BAD_DEPTHS = {
    "nan_row": ((NAN, 0, 0, 0), 0.0, 1.0, 1),
    "inf_row": ((0, 0, 0, -INF), 0.0, 1.0, 1),
    "nan_min": ("cr", NAN, 1.0, 1),
    "inf_max": ("cr", 0.0, INF, 1),
    "min_is_max": ("cr", 1.0, 1.0, 1),
    "min_above_max": ("cr", 1.0, 0.0, 1),
    "no_slices": ("cr", 0.0, 1.0, 0),
    "negative_slices": ("cr", 0.0, 1.0, -1),
    "too_many_slices": ("cr", 0.0, 1.0, 257),
    "window_wider_than_a_double": ("cr", -1.7e308, 1.7e308, 1),
}


def call(cb, d, *, h=16, variant=None, julia=None, projection=None, threads=0):
    """cb_draw_buddhabrot_depth with pointers that are never followed: the lock-step variant consults no interior map,
    and a launch of no threads launches nothing, so an accepted call returns 0 without touching a device."""
    dims = cb.FractalDimensions.make(16, h)
    it = cb.IterationControl(100, 20)
    p = (C.c_double * 8)(*(cb.IDENTITY_PROJECTION if projection is None else projection))
    c = None if julia is None else (C.c_double * 2)(*julia)
    return cb.lib.cb_draw_buddhabrot_depth(C.byref(dims), 4096, C.byref(it), p, c, None if d is None else C.byref(d), 4096,
                                           threads, 50, None, cb.CB_KERNEL_SIMPLE if variant is None else variant, None)


def test_a_valid_depth_is_accepted(cb):
    assert call(cb, cb.Depth.make("cr", -2.0, 0.5, 64)) == 0
    assert call(cb, cb.Depth.make("cr", -2.0, 0.5, 256)) == 0
    assert call(cb, cb.Depth.make((0.5, -0.25, 1e-3, 7.0), -1e9, 1e9, 1), julia=(-0.8, 0.156)) == 0
    assert call(cb, cb.Depth.make("zi", -2.0, 2.0, 4), variant=cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_POWER(3)) == 0
    assert call(cb, cb.Depth.make("zi", -2.0, 2.0, 4), variant=cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FORMULA("tricorn")) == 0
    assert call(cb, cb.Depth.make("zi", -2.0, 2.0, 4), variant=cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_BURNING_SHIP) == 0


@pytest.mark.parametrize("name", list(BAD_DEPTHS))
def test_bad_depths_are_refused(cb, name):
    assert call(cb, cb.Depth.make(*BAD_DEPTHS[name])) == INVALID


def test_what_the_projected_and_julia_draws_refuse_is_refused(cb):
    good = cb.Depth.make("cr", -2.0, 0.5, 5)
    assert call(cb, None) == INVALID
    assert call(cb, cb.Depth.make("cr", 0.0, 1.0, 256), h=(2**31 - 1) // 256 + 1) == INVALID  # N * h > INT_MAX
    assert call(cb, cb.Depth.make("cr", 0.0, 1.0, 255), h=(2**31 - 1) // 256 + 1) == 0
    assert call(cb, good, projection=(1, 0, 0, 0, 0, NAN, 0, 0)) == INVALID
    assert call(cb, good, julia=(2.5, 0.0)) == INVALID and call(cb, good, julia=(0.0, NAN)) == INVALID
    for variant in (cb.CB_KERNEL_TIMED, cb.CB_KERNEL_FULL_ITERATE, cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_ANTI,
                    cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_FLAG_DRAIN, cb.CB_KERNEL_SIMPLE | (2 << 12), cb.CB_KERNEL_SIMPLE | (6 << 16),
                    cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_POWER(3) | cb.CB_KERNEL_FLAG_BURNING_SHIP,
                    cb.CB_KERNEL_SIMPLE | cb.CB_KERNEL_POWER(3) | cb.CB_KERNEL_FORMULA(1)):
        assert call(cb, good, variant=variant) == INVALID, hex(variant)
    dims = cb.FractalDimensions.make(16, 16)
    it = cb.IterationControl(100, 20)
    p = (C.c_double * 8)(*cb.IDENTITY_PROJECTION)
    args = lambda hist, states, pp=p: (C.byref(dims), hist, C.byref(it), pp, None, C.byref(good), states, 0, 50, None,  # noqa: E731
                                       cb.CB_KERNEL_SIMPLE, None)
    assert cb.lib.cb_draw_buddhabrot_depth(*args(None, 4096)) == INVALID
    assert cb.lib.cb_draw_buddhabrot_depth(*args(4096, None)) == INVALID
    assert cb.lib.cb_draw_buddhabrot_depth(*args(4096, 4096, None)) == INVALID
    assert cb.lib.cb_draw_buddhabrot_depth(*args(4096, 4096)) == 0
    assert cb.lib.cb_renderer_set_depth(None, C.byref(good)) == INVALID and cb.lib.cb_renderer_depth(None, None) == 0
    assert cb.lib.cb_renderer_depth_image(None, 1.0, 0, None, None, None) == INVALID
