"""The cell grid's device code -- draw_cells.h's six-draw source (next_sample<true>) and mask sink (mark_cell), PlotMode's
exact map column (draw_plot.h, interior_marked<true>) and the probes' replay accounting -- on PLANTED samples: the first
sample of every subsequence is chosen to the bit (tests/planted_samples.py, its third part): an entry draw either side of a
boundary of j; offset draws 0 and 2^53 - 1; a corner + offset on a tie of the result's format; a c_re one ulp below a marked
cell of the interior map; adjacent doubles across the cardioid's and the bulb's edge, off the grid of the normal stream; a
sample on a cell's edge that sets bit 0 or 31 of the first or last word of the mask; a replay whose first point on the canvas
is z_1, the escaping point, a round's or a chunk's edge, or none.  The generator's own samples reach none of these;
tests/test_planted_cells_host.py shows on the restatements alone that the planted ones do, and that a neighbour of each
plant gives another result.

Every case holds the product kernel to the lock-step kernel and both to the CPU restatement on the same planted states, bit
for bit: histogram or mask words (between guard words, which stay zero), the counters of SAME, status 0 and the generator
states after the run -- the focused render's kernels 6 and 7 (tests/focus_reference.c) and the aimed render's 30 and 31
(tests/aim_reference.c).  A cell-sourced c is read off the aimed draw on --plane cr,ci, where every plotted point is c
itself, on a canvas whose pixels are one ulp wide: the sample is alone in the centre pixel, where the Fraction reference of
the mapping (planted_samples.exact_point) puts it.  No tolerance appears anywhere.

64 subsequences (the planted one in lane 0, in lane 63, in all 64; the others idle on fillers), or the ragged counts of the
last section; one sample per subsequence, and once 49 of the generator's own behind it; canvases of 64 x 48; max_iter at
most 180."""

import numpy as np
import pytest

import aim_harness
import aim_reference as aim
import focus_reference as focus
import planted_samples as P
from aim_harness import aref  # noqa: F401
from device_launches import SAME, assert_same, planar_states
from plot_harness import ref  # noqa: F401
from test_gpu_focus import gpu_launches as focus_launches

pytestmark = pytest.mark.gpu

W, H = 64, 48
CENTRE = (H // 2, W // 2)
GUARD = P.GUARD_WORDS
FOCUS_PRODUCT, FOCUS_LOCKSTEP = 6, 7


def focus_bases(cb):
    return ((cb.CB_KERNEL_DEFAULT, FOCUS_PRODUCT), (cb.CB_KERNEL_SIMPLE, FOCUS_LOCKSTEP))


def drawn(cb, aref, level, cells, draws, box, launches=(1,), max_iter=P.CELL_MAX_ITER, focus_box=P.WIDE_BOX):
    """One planted six-draw sample per subsequence, through the aimed draw of --plane cr,ci on `box` and through the focused
    draw on `focus_box`: product == lock-step == restatement -> (the aimed histogram, its counters, the aimed product
    kernel's counters, the interior map's level at that launch)."""
    states = P.plant_cell_states(draws)
    kw = dict(w=W, h=H, box=box, max_iter=max_iter, min_iter=0, threads=len(draws), level=level, draw=tuple(launches),
              projection=P.C_PLANE)
    st = states.copy()
    want, wc = aim.draw(aref, cells, states=st, **kw)
    assert wc["samples"] == len(draws) * sum(launches) and int(want.sum()) == wc["increments"]
    product = map_level = None
    for lockstep, kernel in aim_harness.BASES:
        hist, cnt, launched, after = aim_harness.gpu_draw(cb, lockstep, cells, states=states, **kw)
        assert launched == kernel
        aim_harness.same_counters(cnt, wc, ("aimed draw", kernel))
        assert np.array_equal(hist, want), ("aimed draw", kernel)
        assert np.array_equal(after, planar_states(st)), ("aimed draw", kernel)
        if lockstep:
            assert cnt["skipped_steps"] == 0
        else:
            product, map_level = cnt, cb.lib.cb_debug_interior_map_level()
    st = states.copy()
    fwant, fwc = focus.draw(aref.focus, W, H, max_iter, 0, len(draws), list(launches), box=focus_box, level=level,
                            cell_list=cells, states=st)
    for base, kernel in focus_bases(cb):
        hist, cnt, launched, after = focus_launches(cb, W, H, focus_box, max_iter, 0, len(draws), list(launches), base,
                                                    level=level, cell_list=cells, states=states)
        assert launched == kernel
        assert_same((hist, cnt), (fwant, fwc), what="focused draw %d" % kernel)
        assert np.array_equal(after, planar_states(st)), ("focused draw", kernel)
    return want, wc, product, map_level


def probed(cb, aref, points, level, box, max_iter, min_iter, launches=(1,), **kw):
    """One planted four-draw sample per subsequence through the probes, the mask between guard words: the aimed probe's
    product == lock-step == restatement and, where the focused probe is defined (no keyword: the Mandelbrot step on a
    sampled c, escaping orbits, the identity plane), the same of its kernels against its restatement and the aimed one's ->
    (mask, counters)."""
    states, n = P.plant_states(points), len(points)
    shape = dict(w=W, h=H, box=box, max_iter=max_iter, min_iter=min_iter, threads=n, level=level, probe=tuple(launches), **kw)
    st = states.copy()
    mask, wc = aim.probe(aref, states=st, **shape)
    if kw.get("bounded"):
        m1, c1 = aim.probe(aref, mode=aim.COMPRESSED, states=states.copy(), **shape)
        assert np.array_equal(m1, mask) and {k: c1[k] for k in SAME} == {k: wc[k] for k in SAME}

    def same(got, cnt, launched, after, kernel):
        assert launched == kernel
        assert not got[:GUARD].any() and not got[-GUARD:].any(), ("guard words", kernel)
        assert np.array_equal(got[GUARD:-GUARD], mask), ("mask", kernel)
        aim_harness.same_counters(cnt, wc, ("probe", kernel))
        assert np.array_equal(after, planar_states(st)), ("probe", kernel)

    for lockstep, kernel in aim_harness.BASES:
        same(*aim_harness.gpu_probe(cb, lockstep, states=states, guard=GUARD, **shape), kernel)
    if not kw:
        m2, c2 = focus.probe(aref.focus, W, H, max_iter, min_iter, n, list(launches), level, box, states=states.copy())
        assert np.array_equal(m2, mask) and c2 == {k: wc[k] for k in c2}
        for base, kernel in focus_bases(cb):
            same(*focus_launches(cb, W, H, box, max_iter, min_iter, n, list(launches), base, level=level, probe=True,
                                 states=states, guard=GUARD), kernel)
    return mask, wc


def alone_in(hist, pixel):
    return hist[pixel] > 0 and int(hist.sum()) == int(hist[pixel])


def only_bits(mask, level, *samples):
    want = np.zeros_like(mask)
    for s in samples:
        word, bit = P.mask_bit(level, *s)
        want[word] |= np.uint32(1 << bit)
    return np.array_equal(mask, want)


def shape_of(k):
    return P.SHAPES[k % len(P.SHAPES)]


# ---- A. the cell-list source ----------------------------------------------------------------------------------------------------


def entry_case(cb, aref, name, threads, launches):
    """The entry plants of a list, cycled through the subsequences: on the whole plane as a canvas the histogram of the first
    launch has the pixels of the selected cells' middles, by exact_entry, and no other."""
    level, cells, plants = P.entry_plants(name)
    draws = [plants[(k + threads) % len(plants)][0] for k in range(threads)]
    want, wc, _, _ = drawn(cb, aref, level, cells, draws, P.SQUARE_C, launches)
    if tuple(launches) == (1,):
        points = [P.exact_sample(level, cells, *d)[1:] for d in draws]
        col, row, ok = P.pixels(P.SQUARE_C, W, H, [p[0] for p in points], [p[1] for p in points])
        assert ok.all() and set(zip(*np.nonzero(want))) == set(zip(row.tolist(), col.tolist()))
        assert wc["recorded"] == threads                                       # cells outside the set, min_iter 0
    return wc


@pytest.mark.parametrize("name", list(P.LIST_SIZES))
def test_the_entry_draw_on_the_edges_of_j(cb, aref, name):
    """ab = 0 and 2^64 - 1, and ceil(k 2^64 / n) - 1 and ceil(k 2^64 / n) for k = 1 and n - 1, on lists of 1, 2, 3, 7, a prime
    near 10^6 and the whole level-10 grid, whose neighbouring entries are cells far apart; then once with 49 samples of the
    generators' own behind the planted one."""
    entry_case(cb, aref, name, 64, (1,))
    wc = entry_case(cb, aref, name, 64, (1, 49))
    assert wc["samples"] == 64 * 50


@pytest.mark.parametrize("level", [4, 10])
def test_offset_draws_zero_and_all_ones(cb, aref, level):
    """v = 0 and v = 2^53 - 1 on either axis: the smallest offset beside a corner 0, the next cell's corner, and c = 2 exactly
    on re, on im and on both from the last column, row and cell."""
    for k, (name, cells, draws, _) in enumerate(P.offset_plants(level)):
        _, re, im = P.exact_sample(level, cells, *draws)
        want, wc, _, _ = drawn(cb, aref, level, cells, P.cell_lanes(draws, shape=shape_of(k)), P.ulp_canvas(re, im))
        assert alone_in(want, CENTRE) and wc["recorded"] == 64, name


@pytest.mark.parametrize("axis", [0, 1], ids=["re", "im"])
@pytest.mark.parametrize("level", [4, 10])
def test_corner_plus_offset_is_rounded_once(cb, aref, level, axis):
    """Exact sums on a tie of the result's format (both parities of the kept bit) and one unit of the offset either side, in
    cells with corner in [-2, -1), [-1, -1/2) and [1/2, 1); the cells with corner -2^-L and 0, where the sum is exact.  The
    sample is alone in the centre pixel of a canvas of one-ulp pixels around the Fraction reference's value: a sum rounded
    twice, or to the other side of a tie, is in the pixel beside it."""
    for k, (name, cells, draws, _, what) in enumerate(P.tie_plants(level, axis)):
        point = P.exact_point(level, int(cells[0]), *draws[1:])
        shapes = P.SHAPES if what == "tie" else (shape_of(k),)
        for shape in shapes:
            want, wc, _, _ = drawn(cb, aref, level, cells, P.cell_lanes(draws, shape=shape), P.ulp_canvas(*point))
            assert alone_in(want, CENTRE) and wc["recorded"] == 64, (name, what, shape)
    name, cells, draws, _, _ = P.tie_plants(level, axis)[1]
    drawn(cb, aref, level, cells, P.cell_lanes(draws, shape="all64"), P.SQUARE_C, (1, 49))


def test_the_map_is_looked_up_in_the_column_that_holds_c(cb, aref):
    """c_re = E - ulp, the largest double below a marked cell's left edge E in (-1, 0): c_re + 2 rounds up to E + 2, the marked
    column, and the cell that holds c is the unmarked one beside it; and c_re = E.  max_iter 100: no periodicity early-out.
    By 98e2ff7 the outside neighbours of marked cells do not escape within 1000 steps, so neither lane escapes, the
    histograms are empty and every counter the restatement has is the same for both: skipped_steps of the product kernel is
    the observable.  Below E the sample is iterated, 100 steps made and none skipped; on E it is retired by the map, all
    100 skipped."""
    for e, im, cells, below, on, map_level in P.map_plants():
        for k, (draws, skipped) in enumerate(((below, 0), (on, 100))):
            for shape in P.SHAPES:
                lanes = 64 if shape == "all64" else 1
                _, wc, product, level = drawn(cb, aref, 10, cells, P.cell_lanes(draws, shape=shape), P.SQUARE_C, max_iter=100)
                assert level == map_level                                      # the product launch consulted the map
                assert (wc["never_escaped"], wc["rejected"], wc["iterate_steps"]) == (lanes, 0, 100 * lanes + 64 - lanes)
                assert product["skipped_steps"] == skipped * lanes, (e, shape, product)


def test_rejection_of_samples_off_the_grid_of_the_normal_stream(cb, aref):
    """Adjacent doubles in c_re, at an ulp finer than 2^-51, one inside and one outside the cardioid, likewise the bulb."""
    for k, (shape, cells, inside, outside, _, _) in enumerate(P.shape_plants()):
        for draws, rejected in ((inside, 1), (outside, 0)):
            for lanes_shape in (shape_of(k), "all64"):
                lanes = 64 if lanes_shape == "all64" else 1
                _, wc, _, _ = drawn(cb, aref, 10, cells, P.cell_lanes(draws, shape=lanes_shape), P.SQUARE_C)
                assert wc["rejected"] == rejected * lanes, (shape, lanes_shape)


# ---- B. the mask sink -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("level", [4, 10])
def test_a_sample_on_a_cell_edge_sets_the_bit_of_its_cell(cb, aref, ref, level):
    """c = -2 + k 2^-L exactly and its grid neighbour below, on each axis, with k chosen for bit 0 and bit 31, the first word
    and the last; c = 2 on re, on im and on both, clamped into the last cell.  (-2 itself cannot be planted: the normal
    stream's least sample is -2 + 2^-51, planted as "the first cell".)  The canvas is around z_1 of the sample."""
    for k, (name, s) in enumerate(P.cell_edge_samples(level)):
        shape = shape_of(k)
        box = P.box_around(P.z_1(ref, s))
        both = P.filler_marks(box) and shape != "all64"                        # the fillers' z_1 beside the sample's: the last cell
        mask, wc = probed(cb, aref, P.lanes(s, 64, shape), level, box, P.CELL_MAX_ITER, 0)
        assert only_bits(mask, level, s, *([P.FILLER] if both else [])), name
        assert (wc["recorded"], wc["replay_steps"]) == (64 if shape == "all64" or both else 1, 64), name


def test_under_a_fixed_c_the_bit_is_the_cell_of_z_0(cb, aref, ref):
    z0 = P.with_end(ref, 13, P.FIXED_C)
    for level in (6, 10):
        for shape in P.SHAPES:
            mask, wc = probed(cb, aref, P.lanes(z0, 64, shape), level, P.WIDE_BOX, 20, 1, c=P.FIXED_C)
            lanes = 64 if shape == "all64" else 1
            assert only_bits(mask, level, z0) and (wc["recorded"], wc["replay_steps"]) == (lanes, lanes)


def test_the_replay_ends_at_the_first_point_on_the_canvas(cb, aref, ref):
    """The first on-canvas point is z_1, the escaping point, the last step of a round or of a chunk or the first of the next,
    or there is none: replay_steps is the marking point's index summed over the lanes (the fillers replay their one point,
    off the canvas), by the restatement and by this closed form."""
    for k, (name, sample, end, box, t) in enumerate(P.replay_cases(ref)):
        for shape in (P.SHAPES if t in (None, 1, 12, 13, 121) else (shape_of(k),)):
            lanes = 64 if shape == "all64" else 1
            mask, wc = probed(cb, aref, P.lanes(sample, 64, shape), 6, box, end + 7, 0)
            assert wc["replay_steps"] == lanes * (end if t is None else t) + 64 - lanes, (name, shape)
            assert wc["recorded"] == (0 if t is None else lanes) and only_bits(mask, 6, *([] if t is None else [sample]))


def test_samples_that_are_too_fast_never_escape_or_are_rejected_mark_nothing(cb, aref, ref):
    """One accepted sample in five among samples that are too fast, never escape or are rejected, every orbit with points on
    the canvas: the mask has the accepted sample's bit alone; without it, none.  The orbits are the cusp's and the neck's:
    the accepted sample's z_1 is on the canvas, so its replay is one step."""
    (max_iter, min_iter), marker, others = P.unmarking_samples(ref)
    for level in (4, 10):
        points = P.cycled([marker] + others, 64)
        mask, wc = probed(cb, aref, points, level, P.WIDE_BOX, max_iter, min_iter)
        n = points.count(marker)
        assert only_bits(mask, level, marker) and (wc["recorded"], wc["replay_steps"]) == (n, n)
        mask, wc = probed(cb, aref, P.cycled(others, 64), level, P.WIDE_BOX, max_iter, min_iter)
        assert not mask.any() and (wc["recorded"], wc["replay_steps"]) == (0, 0)
        # and once with 49 samples of the generators' own behind the planted one: the three-way comparison alone
        _, wc = probed(cb, aref, points, level, P.WIDE_BOX, max_iter, min_iter, launches=(1, 49))
        assert wc["samples"] == 64 * 50 and wc["recorded"] > n


@pytest.mark.parametrize("case", P.BOUNDED_MARKS, ids=lambda c: c[0])
def test_the_bounded_probe_marks_at_the_first_point_of_transient_or_period(cb, aref, case):
    """Orbits that repeat bit for bit, so that the probe replays transient and one period: the first on-canvas point in the
    transient, in the period, the saved point itself; and each orbit again on a canvas it never enters, its cycle found at
    120 of 180 steps -- no bit, recorded 0, the full replay_steps."""
    name, step, c, sample, box, t = case
    m = P.BOUNDED_MAX_ITER
    for shape in P.SHAPES:
        lanes = 64 if shape == "all64" else 1
        for canvas, at in ((box, t), (P.NOWHERE, None)):
            mask, wc = probed(cb, aref, P.lanes(sample, 64, shape), 6, canvas, m, 0, bounded=True, c=c, **step)
            assert (wc["never_escaped"], wc["too_fast"]) == (lanes, 64 - lanes)
            assert wc["replay_steps"] == lanes * (m if at is None else at) and wc["recorded"] == (0 if at is None else lanes)
            assert only_bits(mask, 6, *([] if at is None else [sample])), (name, canvas)


# ---- C. thread counts -----------------------------------------------------------------------------------------------------------

EVERY_Z_1 = (-16.0, 16.0, -12.0, 12.0)             # |z_1| <= |c|^2 + |c| < 11: z_1 of every sample is on it


@pytest.mark.parametrize("threads", [1, 63, 65, 257])
def test_ragged_thread_counts(cb, aref, threads):
    """The entry plants and the cell-edge samples at 1, 63, 65 and 257 subsequences: part of a wave, a wave and a lane, a
    block and a lane."""
    entry_case(cb, aref, "prime", threads, (1,))
    samples = [s for _, s in P.cell_edge_samples(4)]
    points = [samples[(k + threads) % len(samples)] for k in range(threads)]
    mask, wc = probed(cb, aref, points, 4, EVERY_Z_1, P.CELL_MAX_ITER, 0)
    assert only_bits(mask, 4, *points) and (wc["recorded"], wc["replay_steps"]) == (threads, threads)
