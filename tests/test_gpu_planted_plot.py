"""The plotted product kernels (projected with its steps, Julia, palette, depth, depth palette: draw_rounds.h's run_rounds
with the modes of draw_plot.h and draw_depth.h) and their lock-step kernels on PLANTED samples: the first sample of every
subsequence is chosen to the bit (tests/planted_samples.py) -- an orbit that escapes at a round's or a chunk's last step or
the next one's first, either side of max_iter and min_iter; an orbit on |z|^2 == 4 exactly; an orbit that repeats bit for
bit; a c_re on a slice's boundary and the grid point below it; a c on a pixel's or the canvas's edge; a k at a table's first
and last entry.  The generator's own samples reach none of these; tests/test_planted_plot_host.py shows on the restatement
alone that the planted ones do.  The frames and the bounded render are tests/test_gpu_planted_queue.py's.

Every case is plot_harness.three_ways on planted states: product == lock-step == restatement, bit for bit on histogram,
the counters of SAME, the generator states after the run and status 0; where the host file derives a figure directly, it
is asserted on the device's result as well.  64 subsequences (one wave of a ragged block), or 512; launches of one sample --
the planted one alone, the other lanes idle on fillers -- and once (1, 50); canvases of 64 x 48; max_iter at most 1000."""

import numpy as np
import pytest

import plot_harness
import planted_samples as P
import plot_reference as plot
from plot_harness import SQUARE, ref  # noqa: F401

pytestmark = pytest.mark.gpu

W, H = 64, 48
# (product, lock-step) of cb_debug_last_draw_kernel
PROJECTED, POWER, JULIA, PALETTE, FORMULA = (8, 9), (10, 11), (12, 13), (14, 15), (16, 17)
DEPTH, DEPTH_PALETTE = (18, 19), (20, 21)
FAMILIES = {  # the scheduler's: the Mandelbrot step, a step that rejects nothing, a fixed c
    "mandelbrot": (PROJECTED, {}, None),
    "ship": (PROJECTED, dict(ship=True), None),
    "julia": (JULIA, {}, P.FIXED_C),
}


def kernels_of(step, c):
    return JULIA if c is not None else FORMULA if step.get("formula") else POWER if step.get("degree", 2) != 2 else PROJECTED


def three(cb, ref, oracle, kernels, points, max_iter, min_iter, launches=(1,), *, box=SQUARE, **kw):
    """plot_harness.three_ways on planted first samples, at this suite's canvas."""
    mandelbrot = kw.get("c") is None and not kw.get("ship") and not kw.get("formula") and kw.get("degree", 2) == 2
    map_level = 1 if mandelbrot and P.consults_the_map(max_iter, min_iter) else 0
    return plot_harness.three_ways(cb, ref, oracle, kernels, map_level, W, H, box, max_iter, min_iter, len(points), launches,
                                   states=P.plant_states(points), **kw)


# ---- the round scheduler ------------------------------------------------------------------------------------------------------


MORE_STEPS = {**{name: (POWER, step, None) for name, step in P.POWER_STEPS.items()},   # degrees 3 .. 8: power_step_n<D>
              **{name: (FORMULA, step, None) for name, step in P.FORMULA_STEPS.items()}}  # the five formula_step<F>


@pytest.mark.parametrize("end", P.ENDS)
@pytest.mark.parametrize("family", list(FAMILIES) + list(MORE_STEPS))
def test_an_escape_at_a_round_or_chunk_edge_either_side_of_the_window(cb, ref, oracle, family, end):
    """`end` = 1, 12, 13, 60, 61, 120, 121 against kRound = 12 and kChunk = 60, with k = end - 1 the last k accepted
    (max_iter = end), never escaping (max_iter = end - 1), accepted (min_iter = end - 1) and too fast (min_iter = end): alone
    in lane 0, alone in lane 63, in all 64 lanes."""
    kernels, step, c = {**FAMILIES, **MORE_STEPS}[family]
    sample = P.with_end(ref, end, c, **step)
    for max_iter, min_iter, fate in P.windows_of(end):
        for shape in P.SHAPES:
            points = P.lanes(sample, 64, shape)
            r = three(cb, ref, oracle, kernels, points, max_iter, min_iter, c=c, **step)
            model = P.model_counters([end if p == sample else 1 for p in points], max_iter, min_iter)
            assert {k: r.product[k] for k in model} == model, (family, end, max_iter, min_iter, shape)
            assert r.product["skipped_steps"] == 0


@pytest.mark.parametrize("family", list(FAMILIES) + list(MORE_STEPS))
def test_planted_ends_followed_by_the_generators_own_samples(cb, ref, oracle, family):
    """Every end of the list, cycled through 512 subsequences (two whole blocks), then 50 samples of the generators' own;
    under every Multibrot degree and every formula too."""
    kernels, step, c = {**FAMILIES, **MORE_STEPS}[family]
    points = P.cycled([P.with_end(ref, end, c, **step) for end in P.ENDS], 512)
    r = three(cb, ref, oracle, kernels, points, 121, 12, (1, 50), c=c, **step)
    assert r.wc["recorded"] > 512 * 4 // 7


@pytest.mark.parametrize("max_iter", [119, 120, 121, 180])
@pytest.mark.parametrize("case", range(len(P.REPEATING)), ids=lambda k: "%d" % k)
def test_orbits_that_repeat_bit_for_bit_and_orbits_on_the_circle(cb, ref, oracle, case, max_iter):
    """Period 1 and 2, c = -2's two orbits on |z|^2 == 4 among them (the strict m > 4.0 keeps them): never escaping, seen to
    repeat at k = 120 against the point saved at 60, so that the product kernel skips max_iter - 120 steps of each and the
    lock-step kernel none."""
    step, c, sample = P.REPEATING[case]
    (found,) = [f for f in P.repeating(ref, step, c) if f[0] == sample]
    for shape in ("lane0", "all64"):
        points = P.lanes(sample, 64, shape)
        n = points.count(sample)
        r = three(cb, ref, oracle, kernels_of(step, c), points, max_iter, 1, c=c, **step)
        assert r.product["never_escaped"] == n and r.product["too_fast"] == 64 - n and r.product["recorded"] == 0
        assert r.product["skipped_steps"] == n * max(max_iter - 120, 0)
        assert r.extra["chunk_repeats"] == (n if max_iter > 120 else 0)


# ---- slices -------------------------------------------------------------------------------------------------------------------


def planted_in_slices(ref, name):
    """[(sample, slice or None)] of a window: both members of every pair, and the points where the two paths differ."""
    lo, hi, n = P.SLICE_WINDOWS[name]
    edges = P.slice_edges(ref, (lo, hi, n))
    pairs = edges["pairs"] if n <= 8 else edges["pairs"][:2] + edges["pairs"][-2:]
    out = []
    for j, below, above, sb, sa in pairs:
        c_im, _ = P.accepted_beside(ref, (below, above))
        out += [((below, c_im), sb), ((above, c_im), sa)]
    for c_re, s, _ in edges["disagree"]:
        out.append(((c_re, P.accepted_beside(ref, (c_re,))[0]), s))
    return (lo, hi, n), out


@pytest.mark.parametrize("name", list(P.SLICE_WINDOWS))
def test_a_c_re_on_a_slice_boundary_and_the_grid_point_below_it(cb, ref, oracle, name):
    """slice_of's d < min, s < slices and either arithmetic path with the row `cr`, where d is the sample's c_re exactly: the
    lone orbit's increments sit in the plane the host file names and in no other."""
    (lo, hi, n), planted = planted_in_slices(ref, name)
    for sample, s in planted:
        r = three(cb, ref, oracle, DEPTH, P.lanes(sample), 500, 1, box=P.WIDE_BOX, depth=("cr", lo, hi, n))
        assert r.product["recorded"] == 1
        sums = [int(p.sum()) for p in r.want]
        assert sums == [r.product["increments"] if k == s else 0 for k in range(n)] and (s is None or sums[s] > 0)


TABLE_8 = np.array([0x00FFFFFF, 0, 0x010203, 0xFF0000, 0x00FF00, 0x0000FF, 0x7F0080, 0x000100], dtype=np.uint32)


def depth_tables():
    """{window: (table, table with bits 24 to 31 set)}: weights 255, a zero entry, every plane alone; one slice; and 256
    slices staged by threadIdx.x, whose first and last entries differ from every other."""
    most = plot.demo_table(256)
    most[0], most[255] = 0x030201, 0xFFFEFD
    tables = {"reciprocal_8": TABLE_8, "one": np.array([0x0300FF], dtype=np.uint32), "most": most}
    return {k: (t, t | ((np.arange(len(t), dtype=np.uint32) * 37 + 0xA5) << np.uint32(24))) for k, t in tables.items()}


@pytest.mark.parametrize("name", ["reciprocal_8", "one", "most"])
def test_a_planted_slice_takes_its_entry_of_the_table(cb, ref, oracle, name):
    """The depth palette's table by slice: a zero entry for the planted slice (the orbit adds nothing), weights 255, bits 24 to
    31 set on the device's copy alone, one slice, and 256 slices with the orbit in slices 0 and 255."""
    lut, dirty = depth_tables()[name]
    (lo, hi, n), planted = planted_in_slices(ref, name)
    assert {s for _, s in planted} >= ({None, 0, 255} if name == "most" else set(range(n)) | {None})
    for sample, s in planted:
        r = three(cb, ref, oracle, DEPTH_PALETTE, P.lanes(sample), 500, 1, box=P.WIDE_BOX, depth=("cr", lo, hi, n), lut=lut,
                  device_lut=dirty)
        on_canvas = 0 if s is None else int(r.extra["planes"][s].sum())
        assert s is None or on_canvas > 0
        weights = [0, 0, 0] if s is None else [int(w) for w in plot.weights(lut)[s]]
        assert [int(p.sum()) for p in r.want] == [on_canvas * w for w in weights]
        assert r.product["increments"] == on_canvas * sum(weights) and r.product["recorded"] == 1


# ---- pixels -------------------------------------------------------------------------------------------------------------------


def test_a_c_on_a_pixel_edge_and_the_grid_point_below_it(cb, ref, oracle):
    """pixel_of behind project_point with plot.C_PLANE on dyadic pixels: (u, v) is c exactly, so all `end` increments of an
    orbit move at once -- on min and a step below it, on an inner edge and below, on max and below, in x and in y."""
    samples = []
    for axis, name, on, below in P.c_plane_edges(P.C_BOX, W, H):
        n = (W, H)[axis]
        want = {"min": (0, None), "inner": (n // 3, n // 3 - 1), "max": (None, n - 1)}[name]
        for coordinate, index in zip((on, below), want):
            sample = P.c_plane_sample(axis, coordinate)
            samples.append(sample)
            r = three(cb, ref, oracle, PROJECTED, P.lanes(sample, shape="lane63"), 1000, 1, box=P.C_BOX, projection=plot.C_PLANE)
            end = P.end_of(ref, sample, 200)
            assert r.product["recorded"] == 1 and r.product["replay_steps"] == end
            if index is None:
                assert r.product["increments"] == 0
            else:
                row, col = np.argwhere(r.want)[0]
                assert int(r.want[row, col]) == end == r.product["increments"] and (col, row)[axis] == index
    three(cb, ref, oracle, PROJECTED, P.cycled(samples, 512), 1000, 1, (1, 50), box=P.C_BOX, projection=plot.C_PLANE)


def test_an_orbit_point_on_a_border_of_an_irrational_projection(cb, ref, oracle):
    """plot.HOLOGRAM: canvases with an orbit point exactly on their lower bounds, one ulp below them, exactly on their upper
    bounds, and with points that the reciprocal would bin differently from the division."""
    sample, (u, v), canvases = P.hologram_canvases(ref, W, H)
    boxes = [b for kind in ("on_min", "below_min", "on_max", "fallback") for b in canvases[kind]]
    assert len(boxes) >= 3
    for box in boxes:
        for shape in ("lane0", "all64"):
            points = P.lanes(sample, 64, shape)
            r = three(cb, ref, oracle, PROJECTED, points, 61, 1, box=box, projection=plot.HOLOGRAM)
            assert np.array_equal(r.want, P.histogram(box, W, H, u, v) * np.uint64(points.count(sample)))


# ---- palette ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", [None, P.FIXED_C], ids=["sampled", "fixed"])
def test_a_planted_k_at_the_first_and_last_entry_it_can_take(cb, ref, oracle, c):
    """lut[l.end - 1] at k = min_iter and k = max_iter - 1, with distinct entries there and beside; bits 24 to 31 set on the
    device's copy alone; a zero entry at the planted k: the product kernel's skipped_steps grows by `end` and the histogram
    gets nothing."""
    max_iter, min_iter = 61, 12
    lut = plot.demo_table(max_iter)
    dirty = lut | np.uint32(0xC3000000)
    for end, fate in ((12, "too_fast"), (13, "recorded"), (61, "recorded"), (62, "never_escaped")):
        sample = P.with_end(ref, end, c)
        for shape in ("lane0", "all64"):
            points = P.lanes(sample, 64, shape)
            n = points.count(sample)
            r = three(cb, ref, oracle, PALETTE, points, max_iter, min_iter, c=c, lut=lut, device_lut=dirty)
            assert r.product[fate] >= n and r.product["recorded"] == (n if fate == "recorded" else 0)
            assert r.product["skipped_steps"] == 0
            if fate != "recorded":
                assert not r.want.any()
                continue
            plain = three(cb, ref, oracle, JULIA if c else PROJECTED, points, max_iter, min_iter, c=c)
            assert plain.wc["increments"] > 0
            assert all(np.array_equal(p, plain.want * w) for p, w in zip(r.want, plot.weights(lut)[end - 1]))
            for zero in (0, 0xAB000000):
                table = dirty.copy()
                table[end - 1] = zero
                r = three(cb, ref, oracle, PALETTE, points, max_iter, min_iter, c=c, lut=table & np.uint32(0xFFFFFF),
                          device_lut=table)
                assert not r.want.any() and r.product["recorded"] == n and r.extra["zero_entry_steps"] == n * end
                assert r.product["skipped_steps"] == n * end


# ---- cardioid and bulb --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("family", ["projected", "depth"])
def test_cardioid_and_bulb_neighbours_through_the_plotted_kernels(cb, ref, oracle, family):
    """PlotMode::drawn on grid neighbours either side of the two shapes' edges: `rejected` is exactly the inside members."""
    pairs = P.cardioid_pairs(4) + P.bulb_pairs(4)
    assert len(pairs) == 8
    points = P.cycled([p for pair in pairs for p in pair], 512)
    kw = dict(depth=("zr", -2.0, 2.0, 4)) if family == "depth" else {}
    for launches in ((1,), (1, 50)):
        r = three(cb, ref, oracle, DEPTH if family == "depth" else PROJECTED, points, 100, 20, launches, **kw)
        if launches == (1,):
            assert r.product["rejected"] == sum(P.rejected(*p) for p in points) == 256
